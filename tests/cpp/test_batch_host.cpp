// Host-only check of csrc/gol_batch_host.h (the argument arithmetic and the packed .NET seeding behind the gol_batch_*
// entry points), with its own main.  Built with -fsanitize=address,undefined by tests/test_batch_host.py: an overflow
// in the range arithmetic or a word written outside a board's rows ends the program.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gameoflifewithactors_amd/csrc/gol_batch_host.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

int main() {
    using namespace gol;
    // ---- geometry
    CHECK(wave_resident_rpl(100, 100) == 2 && wave_resident_rpl(128, 256) == 4 && wave_resident_rpl(3, 3) == 1 &&
          wave_resident_rpl(127, 192) == 3);
    CHECK(wave_resident_rpl(129, 64) == 0 && wave_resident_rpl(128, 255) == 0 && wave_resident_rpl(100, 257) == 0 &&
          wave_resident_rpl(2, 64) == 0);
    CHECK(wave_resident_rpl(INT64_MAX, INT64_MAX) == 0 && wave_resident_rpl(INT64_MIN, 5) == 0 &&
          wave_resident_rpl(100, INT64_MIN) == 0);
    // ... under the rule family: the last lane partly filled where the rows do not divide into lanes
    CHECK(wave_rule_rpl(100, 101) == 2 && wave_rule_rpl(33, 127) == 2 && wave_rule_rpl(96, 190) == 3 &&
          wave_rule_rpl(64, 191) == 3 && wave_rule_rpl(128, 255) == 4 && wave_rule_rpl(5, 253) == 4);
    CHECK(wave_rule_rpl(100, 257) == 0 && wave_rule_rpl(129, 64) == 0);
    CHECK(wave_rule_rpl(INT64_MAX, INT64_MAX) == 0 && wave_rule_rpl(INT64_MIN, 5) == 0 &&
          wave_rule_rpl(100, INT64_MIN) == 0 && wave_rule_rpl(100, INT64_MAX) == 0);
    for (int64_t W = 3; W <= 128; W++)
        for (int64_t H = 3; H <= 256; H++) {
            const int r = wave_resident_rpl(W, H);
            CHECK(r == 0 || wave_rule_rpl(W, H) == r);
        }
    // ---- board ranges: count boards of `cells` cells
    const int64_t cells = 128 * 256, count = kBatchCountMax;
    CHECK(batch_range_ok(0, count, count, count * cells, cells));
    CHECK(batch_range_ok(count - 1, 1, count, cells, cells));
    CHECK(batch_range_ok(2, 2, 6, 2 * cells, cells));
    CHECK(!batch_range_ok(0, 0, count, 0, cells));
    CHECK(!batch_range_ok(-1, 1, count, cells, cells));
    CHECK(!batch_range_ok(count, 1, count, cells, cells));
    CHECK(!batch_range_ok(5, 2, 6, 2 * cells, cells));
    CHECK(!batch_range_ok(2, 2, 6, 2 * cells + 1, cells));
    CHECK(!batch_range_ok(1, INT64_MAX, count, cells, cells));  // first + n would overflow
    CHECK(!batch_range_ok(INT64_MAX, INT64_MAX, count, cells, cells));
    CHECK(!batch_range_ok(INT64_MIN, INT64_MIN, count, INT64_MIN, cells));
    // ---- trace calls
    int64_t samples = -1;
    const char* why = nullptr;
    CHECK(batch_trace_ok(60, 15, 5, 20, &samples, &why) && samples == 4);
    CHECK(batch_trace_ok(0, 3, 5, 0, &samples, &why) && samples == 0);
    CHECK(batch_trace_ok(kBatchTraceMax, 1, 1, kBatchTraceMax, &samples, &why) && samples == kBatchTraceMax);
    CHECK(!batch_trace_ok(kBatchTraceMax + 1, 1, 1, kBatchTraceMax + 1, &samples, &why));
    CHECK(!batch_trace_ok(60, 0, 5, 0, &samples, &why));
    CHECK(!batch_trace_ok(60, -3, 5, 0, &samples, &why));
    CHECK(!batch_trace_ok(60, 7, 5, 40, &samples, &why));
    CHECK(!batch_trace_ok(-60, 15, 5, -20, &samples, &why));
    CHECK(!batch_trace_ok(60, 15, 5, 21, &samples, &why));
    CHECK(!batch_trace_ok(INT64_MAX, 1, count, INT64_MAX, &samples, &why));  // t * count would overflow
    CHECK(batch_trace_ok(INT64_MAX - 6, INT64_MAX - 6, count, count, &samples, &why) && samples == 1);
    CHECK(!batch_trace_ok(INT64_MIN, INT64_MIN, count, 0, &samples, &why));
    // ---- packed seeding: the words are the bytes gol_seed_dotnet writes (x outer, y inner), bits past W zero, and
    // nothing outside the board's H * nw words is touched (guard words around it)
    for (int mode = 0; mode < 2; mode++)
        for (auto wh : {std::pair<int64_t, int64_t>{100, 100}, {33, 12}, {3, 3}, {128, 256}, {32, 64}}) {
            const int64_t W = wh.first, H = wh.second, nw = (W + 31) / 32;
            std::vector<uint32_t> buf((size_t)(H * nw) + 2, 0xA5A5A5A5u);
            batch_seed_dotnet_words(42, mode, W, H, buf.data() + 1);
            CHECK(buf.front() == 0xA5A5A5A5u && buf.back() == 0xA5A5A5A5u);
            std::vector<uint8_t> bytes((size_t)(W * H));
            DotNetRandom r(42);
            for (int64_t x = 0; x < W; x++)
                for (int64_t y = 0; y < H; y++)
                    bytes[(size_t)(x + y * W)] = mode == 0 ? (r.Next() % 2 == 0) : (r.Next(2) == 0);
            for (int64_t y = 0; y < H; y++)
                for (int64_t x = 0; x < 32 * nw; x++) {
                    const uint32_t bit = (buf[(size_t)(1 + y * nw + (x >> 5))] >> (x & 31)) & 1u;
                    CHECK(bit == (x < W ? bytes[(size_t)(x + y * W)] : 0u));
                }
        }
    std::printf("batch host ok\n");
    return 0;
}
