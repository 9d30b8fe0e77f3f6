// Host check of the one-thread code builders of the match-search PNG encoder (gance_amd/csrc/png_lz_codes.h and the
// builders of png_common.h they drive), with the host sanitizers. No GPU is touched: build and run on a CPU,
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/png_lz_codes_check.hip -o /tmp/png_lz_codes_check && /tmp/png_lz_codes_check
// Histograms: one, two and all 30 used distance symbols; a literal/length histogram of Fibonacci counts, whose
// unrestricted code is deeper than 15 bits; one with only end-of-block and one length symbol; every byte value. Checks:
// every Kraft sum is exactly one (a single distance symbol: one code of one bit), no length is over its limit, symbol 256
// has a code, HLIT / HDIST end at the last used symbol, the run-length symbols decode back to the lengths they code, and
// the header's bit count is the number of bits write_lz_head writes; the length and distance symbols against RFC 1951's
// tables at every value.

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
    std::printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
