// Host check of the one-thread code builders of both PNG encoders (gance_amd/csrc/png_common.h: the default encoder's
// plan_segment, write_head_and_tail and code_length_code; gance_amd/csrc/png_lz_codes.h: the match-search encoder's), with
// the host sanitizers. No GPU is touched: build and run on a CPU,
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/png_lz_codes_check.hip -o /tmp/png_lz_codes_check && /tmp/png_lz_codes_check
// tests/test_png_codes.py does so in the suite.
// Match search. Histograms: one, two and all 30 used distance symbols; a literal/length histogram of Fibonacci counts, whose
// unrestricted code is deeper than 15 bits; one with only end-of-block and one length symbol; every byte value. Checks:
// every Kraft sum is exactly one (a single distance symbol: one code of one bit), no length is over its limit, symbol 256
// has a code, HLIT / HDIST end at the last used symbol, the run-length symbols decode back to the lengths they code, and
// the header's bit count is the number of bits write_lz_head writes; the length and distance symbols against RFC 1951's
// tables at every value.
// Default encoder. Byte counts: twenty Fibonacci numbers (depth 19), every byte value (unevenly; evenly, which is stored),
// one byte value, two bytes. Checks: the same of the literal and the code-length code, a more frequent symbol never has the
// longer code, the stored / coded choice and the size are the rule's, and the header, end-of-block and the empty stored
// block read back bit by bit from what write_head_and_tail wrote, ending where the plan says.
// code_length_code alone: counts whose unrestricted code is deeper than 7 bits (9 and 18).

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gance_amd/csrc/png_lz_codes.h"

namespace gance {
int set_last_error(int code, const std::string&) { return code; }  // png_common.h's argument checks are not used here
}  // namespace gance

using namespace gance_png;

static int failures = 0;
#define CHECK(condition)                                                     \
    do {                                                                     \
        if (!(condition)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #condition), ++failures; \
        }                                                                    \
    } while (0)

static uint64_t kraft(const uint8_t* lengths, int n, int max_bits, int* used, int* longest) {
    uint64_t sum = 0;
    *used = 0, *longest = 0;
    for (int s = 0; s < n; ++s)
        if (lengths[s]) {
            sum += 1ull << (max_bits - lengths[s]);
            ++*used;
            *longest = std::max(*longest, (int)lengths[s]);
        }
    return sum;
}

static int sort_used(const std::vector<uint32_t>& histogram, uint32_t* sorted, uint16_t* symbols) {
    std::vector<int> order;
    for (int s = 0; s < (int)histogram.size(); ++s)
        if (histogram[s]) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return histogram[a] != histogram[b] ? histogram[a] < histogram[b] : a < b; });
    for (size_t i = 0; i < order.size(); ++i) sorted[i] = histogram[order[i]], symbols[i] = (uint16_t)order[i];
    return (int)order.size();
}

static void check_case(const char* name, std::vector<uint32_t> hist_ll, std::vector<uint32_t> hist_d) {
    hist_ll.resize(kLitLen + 2), hist_d.resize(kDist + 2);
    hist_ll[256] = 1;
    uint32_t sorted_ll[kLitLen + 2], sorted_d[kDist + 2];
    uint16_t symbol_ll[kLitLen + 2], symbol_d[kDist + 2], ll_code[kLitLen + 2] = {}, d_code[kDist + 2] = {}, cl_code[19] = {};
    uint8_t ll_length[kLitLen + 2] = {}, d_length[kDist + 2] = {}, cl_length[19] = {}, run_symbol[kLitLen + kDist], run_extra[kLitLen + kDist];
    const int used_ll = sort_used(hist_ll, sorted_ll, symbol_ll), used_d = sort_used(hist_d, sorted_d, symbol_d);
    const LzPlan plan = plan_lz_segment(hist_ll.data(), sorted_ll, symbol_ll, used_ll, hist_d.data(), sorted_d, symbol_d, used_d, 4, ll_length,
                                        ll_code, d_length, d_code, cl_length, cl_code, run_symbol, run_extra);
    int used, longest;
    CHECK(kraft(ll_length, kLitLen, 15, &used, &longest) == 1ull << 15);
    CHECK(used == used_ll && longest <= 15 && ll_length[256] > 0);
    const uint64_t distance_sum = kraft(d_length, kDist, 15, &used, &longest);
    CHECK(used == used_d && longest <= 15);
    CHECK(used_d == 1 ? (distance_sum == 1ull << 14 && longest == 1) : distance_sum == 1ull << 15);
    CHECK(kraft(cl_length, 19, 7, &used, &longest) == 1ull << 7 && longest <= 7);
    CHECK(plan.hlit >= 257 && plan.hlit <= kLitLen && ll_length[plan.hlit - 1] > 0);
    for (int s = plan.hlit; s < kLitLen; ++s) CHECK(ll_length[s] == 0);
    CHECK(plan.hdist >= 1 && plan.hdist <= kDist && d_length[plan.hdist - 1] > 0);
    for (int s = plan.hdist; s < kDist; ++s) CHECK(d_length[s] == 0);
    for (int s = 0; s < kLitLen; ++s) CHECK((hist_ll[s] > 0) == (ll_length[s] > 0));
    // the run-length symbols decode to the lengths; every symbol sent has a code
    std::vector<int> decoded;
    uint32_t run_bits = 0;
    for (int i = 0; i < plan.runs; ++i) {
        const int symbol = run_symbol[i], extra = run_extra[i];
        CHECK(symbol <= 18 && cl_length[symbol] > 0);
        run_bits += cl_length[symbol] + (symbol == 16 ? 2 : symbol == 17 ? 3 : symbol == 18 ? 7 : 0);
        if (symbol < 16) {
            decoded.push_back(symbol);
        } else if (symbol == 16) {
            CHECK(!decoded.empty() && extra <= 3);
            for (int k = 0; k < 3 + extra && !decoded.empty(); ++k) decoded.push_back(decoded.back());
        } else {
            CHECK(extra <= (symbol == 17 ? 7 : 127));
            decoded.insert(decoded.end(), (symbol == 17 ? 3 : 11) + extra, 0);
        }
    }
    CHECK((int)decoded.size() == plan.hlit + plan.hdist);
    for (int i = 0; i < (int)decoded.size() && i < plan.hlit + plan.hdist; ++i)
        CHECK(decoded[i] == (i < plan.hlit ? ll_length[i] : d_length[i - plan.hlit]));
    CHECK(plan.cl_count >= 4 && plan.cl_count <= 19);
    CHECK(plan.data_bit == 8 * 4 + 17 + 3 * plan.cl_count + (int)run_bits);
    // the header's bits end where the plan says the tokens begin
    std::vector<uint32_t> buffer(256, 0);
    write_lz_head(buffer.data(), plan, 4, cl_length, cl_code, run_symbol, run_extra);
    for (int bit = plan.data_bit; bit < 256 * 32; ++bit) CHECK(((buffer[bit >> 5] >> (bit & 31)) & 1u) == 0);
    CHECK(((buffer[1] >> 1) & 3u) == 2u);  // BTYPE
    std::printf("%-28s lit/len %3d used, HLIT %3d, distance %2d used, HDIST %2d, %3d run symbols, header %4d bits\n", name, used_ll, plan.hlit,
                used_d, plan.hdist, plan.runs, plan.data_bit - 32);
}

// Reads a buffer the way an inflater does: bits LSB first, Huffman codes bit by bit against the canonical code of `lengths`
struct BitReader {
    const uint32_t* words;
    int position;
    uint32_t bits(int count) {
        uint32_t value = 0;
        for (int i = 0; i < count; ++i, ++position) value |= ((words[position >> 5] >> (position & 31)) & 1u) << i;
        return value;
    }
    int symbol(const uint8_t* lengths, int n, int max_bits) {  // -1: no code of up to max_bits bits begins here
        int count[17] = {}, first = 0, code = 0;
        for (int s = 0; s < n; ++s) ++count[lengths[s]];
        count[0] = 0;
        for (int length = 1; length <= max_bits; ++length) {
            code |= (int)bits(1);
            if (code - first < count[length]) {
                int seen = 0;
                for (int s = 0; s < n; ++s)
                    if (lengths[s] == length && seen++ == code - first) return s;
            }
            first = (first + count[length]) << 1;
            code <<= 1;
        }
        return -1;
    }
};

// The default encoder's builders: plan_segment and write_head_and_tail on a literal histogram (end-of-block is added here)
static void check_plan_case(const char* name, std::vector<uint32_t> histogram, int start_bytes, bool last, int want_longest = 0) {
    histogram.resize(kLiterals + 3);
    histogram[256] = 1;
    int n = 0;
    for (int s = 0; s < 256; ++s) n += (int)histogram[s];
    uint32_t sorted[kLiterals + 3];
    uint16_t symbols[kLiterals + 3], lit_code[kLiterals + 3] = {}, cl_code[19] = {};
    uint8_t lit_length[kLiterals + 3] = {}, cl_length[19] = {};
    const int used_symbols = sort_used(histogram, sorted, symbols);
    const SegmentPlan plan = plan_segment(histogram.data(), sorted, symbols, used_symbols, n, start_bytes, lit_length, lit_code, cl_length, cl_code);
    int used, longest;
    CHECK(kraft(lit_length, kLiterals, 15, &used, &longest) == 1ull << 15);
    CHECK(used == used_symbols && longest <= 15 && lit_length[256] > 0);
    const int lit_longest = longest;
    CHECK(want_longest == 0 || lit_longest == want_longest);  // over-long codes go to the limit itself
    for (int s = 0; s < kLiterals; ++s) CHECK((histogram[s] > 0) == (lit_length[s] > 0));
    for (int a = 0; a < kLiterals; ++a)  // a more frequent symbol never has the longer code
        for (int b = 0; b < kLiterals; ++b)
            if (histogram[a] > histogram[b] && histogram[b] > 0) CHECK(lit_length[a] <= lit_length[b]);
    CHECK(kraft(cl_length, 19, 7, &used, &longest) == 1ull << 7 && longest <= 7);
    uint32_t data_bits = 0, length_bits = 0;
    for (int s = 0; s < kLiterals; ++s) data_bits += histogram[s] * lit_length[s], length_bits += cl_length[lit_length[s]];
    CHECK(plan.cl_count >= 4 && plan.cl_count <= 19);
    CHECK(plan.data_bit == 8 * start_bytes + 17 + 3 * plan.cl_count + (int)length_bits + cl_length[1]);
    const int header_bits = plan.data_bit - 8 * start_bytes;
    const int coded_bytes = (header_bits + (int)data_bits + 3 + 7) / 8 + 4;
    CHECK(plan.coded == (coded_bytes <= 5 + n ? 1 : 0));
    CHECK(plan.total_bytes == start_bytes + (plan.coded ? coded_bytes : 5 + n));
    // what write_head_and_tail writes, read back: the header ends where the plan says the literals begin, and behind
    // their bits come end-of-block, the empty stored block on its byte boundary, and nothing more
    std::vector<uint32_t> buffer((start_bytes + coded_bytes) / 4 + 4, 0);  // the stored form's choice is checked above: room for either
    const int all_bits = (int)data_bits - lit_length[256];
    write_head_and_tail(buffer.data(), plan, start_bytes, all_bits, last, lit_length, lit_code, cl_length, cl_code);
    BitReader reader{buffer.data(), 8 * start_bytes};
    CHECK(reader.bits(1) == 0 && reader.bits(2) == 2 && reader.bits(5) == 0 && reader.bits(5) == 0);
    CHECK((int)reader.bits(4) == plan.cl_count - 4);
    uint8_t read_cl[19] = {};
    for (int i = 0; i < plan.cl_count; ++i) read_cl[cl_order(i)] = (uint8_t)reader.bits(3);
    for (int s = 0; s < 19; ++s) CHECK(read_cl[s] == cl_length[s]);
    for (int s = 0; s < kLiterals + 1; ++s) CHECK(reader.symbol(read_cl, 19, 7) == (s < kLiterals ? lit_length[s] : 1));
    CHECK(reader.position == plan.data_bit);
    for (int bit = plan.data_bit; bit < plan.data_bit + all_bits; ++bit) CHECK(((buffer[bit >> 5] >> (bit & 31)) & 1u) == 0);
    reader.position = plan.data_bit + all_bits;
    CHECK(reader.symbol(lit_length, kLiterals, 15) == 256);
    CHECK(reader.bits(1) == (last ? 1u : 0u) && reader.bits(2) == 0);
    while (reader.position & 7) CHECK(reader.bits(1) == 0);
    CHECK(reader.bits(16) == 0 && reader.bits(16) == 0xFFFF);
    CHECK(reader.position == 8 * (start_bytes + coded_bytes));
    for (int bit = reader.position; bit < 32 * (int)buffer.size(); ++bit) CHECK(((buffer[bit >> 5] >> (bit & 31)) & 1u) == 0);
    std::printf("%-28s literals %3d used, longest %2d, %s, header %4d bits, data %6u bits\n", name, used_symbols, lit_longest,
                plan.coded ? "coded" : "stored", header_bits, data_bits);
}

// code_length_code alone, on the counts of the 19 code-length symbols
static void check_cl_case(const char* name, const std::vector<uint32_t>& frequency, int want_longest) {
    uint8_t cl_length[19] = {};
    uint16_t cl_code[19] = {};
    int cl_count = 0;
    const uint32_t bits = code_length_code(frequency.data(), cl_length, cl_code, &cl_count);
    int used, longest, want_used = 0;
    CHECK(kraft(cl_length, 19, 7, &used, &longest) == 1ull << 7 && longest == want_longest);
    uint32_t want_bits = 0;
    for (int s = 0; s < 19; ++s) want_used += frequency[s] > 0, want_bits += frequency[s] * cl_length[s];
    CHECK(used == want_used);
    for (int s = 0; s < 19; ++s) CHECK((frequency[s] > 0) == (cl_length[s] > 0));
    for (int a = 0; a < 19; ++a)
        for (int b = 0; b < 19; ++b)
            if (frequency[a] > frequency[b] && frequency[b] > 0) CHECK(cl_length[a] <= cl_length[b]);
    CHECK(cl_count >= 4 && cl_count <= 19 && (cl_count == 4 || cl_length[cl_order(cl_count - 1)] > 0));
    for (int i = cl_count; i < 19; ++i) CHECK(cl_length[cl_order(i)] == 0);
    CHECK(bits == 3 * (uint32_t)cl_count + want_bits);
    // the codes are the canonical ones of the lengths, bit-reversed: each reads back as its symbol
    for (int s = 0; s < 19; ++s) {
        if (cl_length[s] == 0) continue;
        uint32_t word[2] = {cl_code[s], 0};
        BitReader reader{word, 0};
        CHECK(reader.symbol(cl_length, 19, 7) == s && reader.position == cl_length[s]);
    }
    std::printf("%-28s code-length symbols %2d used, longest %d, %2d lengths sent, %4u bits\n", name, used, longest, cl_count, bits);
}

int main() {
    // RFC 1951 3.2.5
    static const int length_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int length_bits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int length = 3; length <= 258; ++length) {
        int bits, extra;
        const int symbol = length_symbol(length, &bits, &extra);
        CHECK(symbol >= 257 && symbol <= 285 && bits == length_bits[symbol - 257] && length_base[symbol - 257] + extra == length);
        CHECK(extra < (1 << bits) && length_extra_bits(symbol) == bits);
    }
    for (int distance = 1; distance <= 32768; ++distance) {
        int bits, extra;
        const int symbol = distance_symbol(distance, &bits, &extra);
        const int want_bits = symbol < 4 ? 0 : symbol / 2 - 1;
        const int base = symbol < 4 ? symbol + 1 : ((2 + (symbol & 1)) << want_bits) + 1;
        CHECK(symbol >= 0 && symbol <= 29 && bits == want_bits && base + extra == distance && extra < (1 << bits));
        CHECK(distance_extra_bits(symbol) == bits);
    }

    std::vector<uint32_t> few(kLitLen, 0), all(kLitLen, 0), fibonacci(kLitLen, 0), only_length(kLitLen, 0);
    few[0] = 900, few[1] = 40, few[77] = 3, few[285] = 120, few[260] = 2;
    for (int s = 0; s < kLitLen; ++s) all[s] = 1 + (uint32_t)((s * 2654435761u) % 97);
    uint32_t a = 1, b = 1;
    for (int s = 0; s < 21; ++s) {  // 21 Fibonacci counts and end-of-block: an unrestricted code of depth 21
        fibonacci[s < 20 ? 10 * s : 270] = a;
        const uint32_t next = a + b;
        a = b, b = next;
    }
    only_length[285] = 127;
    std::vector<uint32_t> one(kDist, 0), two(kDist, 0), thirty(kDist, 0), skewed(kDist, 0);
    one[0] = 127;
    two[0] = 5, two[17] = 1;
    for (int s = 0; s < kDist; ++s) thirty[s] = 1 + (uint32_t)s, skewed[s] = 1u << (s < 24 ? s : 24);
    one[0] = 127;
    check_case("one distance symbol", few, one);
    {
        std::vector<uint32_t> high(kDist, 0);
        high[29] = 9;
        check_case("one distance symbol, the last", few, high);
    }
    check_case("two distance symbols", few, two);
    check_case("all 30 distance symbols", all, thirty);
    check_case("30 distances, powers of two", all, skewed);
    check_case("Fibonacci literal counts", fibonacci, two);
    check_case("end-of-block and one length", only_length, one);

    // the default encoder: a segment's 256 byte counts
    std::vector<uint32_t> fibonacci_bytes(256, 0), every_byte(256, 0), uniform(256, 8), one_byte(256, 0), two_bytes(256, 0);
    a = 1, b = 2;
    for (int k = 19; k >= 0; --k) {  // 1, 2, 3, 5 ... 10946, the most frequent on value 0, then 1, 255, 2, 254 ...: depth 19 with end-of-block
        fibonacci_bytes[k == 0 ? 0 : (k & 1 ? (k + 1) / 2 : 256 - k / 2)] = a;
        const uint32_t next = a + b;
        a = b, b = next;
    }
    for (int s = 0; s < 256; ++s) every_byte[s] = 1 + (uint32_t)((s * 2654435761u) % 97);
    one_byte[77] = 12288;
    two_bytes[0] = 1, two_bytes[255] = 1;
    check_plan_case("Fibonacci byte counts", fibonacci_bytes, 4, false, 15);
    check_plan_case("Fibonacci, first and last", fibonacci_bytes, 6, true, 15);
    check_plan_case("every byte value", every_byte, 4, false);
    check_plan_case("every byte value, evenly", uniform, 6, true);
    check_plan_case("one byte value", one_byte, 4, true);
    check_plan_case("two bytes", two_bytes, 6, false);

    // the code-length code alone, deeper than 7 bits: the counts of a literal code with the lengths 1 (once), 4 (3), 7 (34),
    // 8 (8), 11 (13), 12 (21), 13 (5), 14 (2), 15 (112), 58 unused symbols and the distance length 1: depth 9; 19 Fibonacci counts
    std::vector<uint32_t> dyadic(19, 0), fibonacci_cl(19, 0), two_cl(19, 0);
    dyadic[0] = 58, dyadic[1] = 2, dyadic[4] = 3, dyadic[7] = 34, dyadic[8] = 8, dyadic[11] = 13, dyadic[12] = 21, dyadic[13] = 5, dyadic[14] = 2;
    dyadic[15] = 112;
    a = 1, b = 2;
    for (int s = 0; s < 19; ++s) {
        fibonacci_cl[(7 * s) % 19] = a;
        const uint32_t next = a + b;
        a = b, b = next;
    }
    two_cl[0] = 200, two_cl[18] = 3;
    check_cl_case("dyadic literal profile", dyadic, 7);
    check_cl_case("19 Fibonacci counts", fibonacci_cl, 7);
    check_cl_case("two code-length symbols", two_cl, 1);
    std::printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
