// Host-only check of the per-board rule table of csrc/gol_batch_host.h (batch_rules_pack, batch_rules_common: what
// gol_ensemble_set_rules and gol_ensemble_rule decide on the host), with its own main.  Built with
// -fsanitize=address,undefined by tests/test_batch_rules_host.py: a word written outside the table, a read past the
// caller's arrays or a shift of a negative mask ends the program.
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

namespace {

constexpr uint32_t kGuard = 0xA5A5A5A5u;

// `packed` with a guard word on each side; `touched` = any word of it differs from the guard pattern
struct Table {
    std::vector<uint32_t> buf;
    explicit Table(int64_t count) : buf((size_t)count + 2, kGuard) {}
    uint32_t* data() { return buf.data() + 1; }
    bool guards() const { return buf.front() == kGuard && buf.back() == kGuard; }
    bool touched() const {
        for (uint32_t v : buf)
            if (v != kGuard) return true;
        return false;
    }
};

}  // namespace

int main() {
    using namespace gol;
    const char* why = nullptr;
    int64_t bad = 7;

    // ---- a valid table: every entry packed as rule_pack packs it, nothing outside the count words written
    for (int64_t count : {(int64_t)1, (int64_t)37, (int64_t)1100}) {
        std::vector<int> birth((size_t)count), survive((size_t)count);
        for (int64_t i = 0; i < count; i++) {
            birth[(size_t)i] = (int)((i * 131) & kRuleMaskMax);
            survive[(size_t)i] = (int)((i * 29 + 5) & kRuleMaskMax);
        }
        Table t(count);
        why = nullptr;
        CHECK(batch_rules_pack(birth.data(), survive.data(), count, count, t.data(), &why, &bad));
        CHECK(why == nullptr && bad == -1 && t.guards());
        for (int64_t i = 0; i < count; i++) {
            const uint32_t p = t.data()[i];
            CHECK(p == rule_pack(birth[(size_t)i], survive[(size_t)i]) && p < (1u << 18));
            CHECK((int)(p & kRuleMaskMax) == birth[(size_t)i] && (int)(p >> 9) == survive[(size_t)i]);
        }
        CHECK(batch_rules_pack(birth.data(), survive.data(), count, count, t.data(), &why));  // bad_index is optional
    }
    // the extremes of the range, and Conway's packed word
    {
        const int birth[3] = {0, kRuleMaskMax, kRuleLifeBirth}, survive[3] = {kRuleMaskMax, 0, kRuleLifeSurvive};
        uint32_t packed[3];
        CHECK(batch_rules_pack(birth, survive, 3, 3, packed, &why));
        CHECK(packed[0] == 0x3FE00u && packed[1] == 0x1FFu && packed[2] == kRuleLifePacked);
    }

    // ---- refusals: `why` set, the table untouched -- a bad mask at the LAST entry too (the whole table is judged
    // before a word is written)
    const int64_t count = 37;
    std::vector<int> birth((size_t)count, 8), survive((size_t)count, 12);
    const auto refused = [&](const int* b, const int* s, int64_t n, int64_t want_bad) {
        Table t(count);
        why = nullptr;
        bad = 7;
        const bool ok = batch_rules_pack(b, s, n, count, t.data(), &why, &bad);
        return !ok && why && why[0] && bad == want_bad && !t.touched();
    };
    CHECK(refused(nullptr, survive.data(), count, -1));
    CHECK(refused(birth.data(), nullptr, count, -1));
    CHECK(refused(nullptr, nullptr, count, -1));
    for (int64_t n : {(int64_t)0, (int64_t)-1, count - 1, count + 1, INT64_MAX, INT64_MIN})
        CHECK(refused(birth.data(), survive.data(), n, -1));  // n != count: the arrays are never read
    for (int mask : {0x200, -1, INT32_MAX, INT32_MIN, 0x1FF + 0x40000})
        for (int64_t at : {(int64_t)0, (int64_t)18, count - 1}) {
            birth[(size_t)at] = mask;
            CHECK(refused(birth.data(), survive.data(), count, at));
            birth[(size_t)at] = 8;
            survive[(size_t)at] = mask;
            CHECK(refused(birth.data(), survive.data(), count, at));
            survive[(size_t)at] = 12;
        }
    birth[3] = -1;  // two bad entries: the first is named
    survive[30] = 0x200;
    CHECK(refused(birth.data(), survive.data(), count, 3));
    birth[3] = 8;
    survive[30] = 12;
    {
        why = nullptr;
        CHECK(!batch_rules_pack(birth.data(), survive.data(), count, count, nullptr, &why) && why);  // no table
    }

    // ---- the common rule of a table
    {
        std::vector<uint32_t> packed((size_t)count, kRuleLifePacked);
        uint32_t rule = 0xFFFFFFFFu;
        CHECK(batch_rules_common(packed.data(), count, &rule) && rule == kRuleLifePacked);
        CHECK(batch_rules_common(packed.data(), 1, &rule) && rule == kRuleLifePacked);
        for (int64_t at : {(int64_t)0, (int64_t)1, count - 1}) {
            packed[(size_t)at] ^= 1u;
            rule = 0xFFFFFFFFu;
            CHECK(!batch_rules_common(packed.data(), count, &rule) && rule == 0xFFFFFFFFu);  // untouched
            packed[(size_t)at] ^= 1u;
        }
        packed[(size_t)(count - 1)] = 0;  // beyond the `count` asked about: not looked at
        CHECK(batch_rules_common(packed.data(), count - 1, &rule) && rule == kRuleLifePacked);
    }
    std::printf("batch rules host ok\n");
    return 0;
}
