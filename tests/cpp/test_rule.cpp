// Host check of life-like rules (gameoflifewithactors_amd/csrc/gol_rule.h, gol_bitlogic.h rule_next), built with the
// address and undefined-behaviour sanitizers and run by tests/test_rule_host.py (CPU):
//   text    format then parse is the identity on all 2^18 rules; the three spellings of a rule parse alike; every
//           malformed text is refused with both outputs untouched
//   rule    the bit-sliced evaluator against the scalar definition (rule_next_cell) on all 2^9 neighbourhoods, packed
//           32 to a word, under all 2^18 rules; under B3/S23 it equals life_next
#include <cstdio>
#include <cstring>
#include <string>

#include "../../gameoflifewithactors_amd/csrc/gol_bitlogic.h"
#include "../../gameoflifewithactors_amd/csrc/gol_rule.h"

static long bad = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            if (bad++ < 20) std::printf("line %d: %s\n", __LINE__, #x); \
        }                                                          \
    } while (0)

static bool parses_to(const char* text, int birth, int survive) {
    int b = -7, s = -7;
    const char* why = nullptr;
    return gol::rule_parse(text, &b, &s, &why) && b == birth && s == survive;
}

static bool refused(const char* text) {
    int b = -7, s = -9;
    const char* why = nullptr;
    return !gol::rule_parse(text, &b, &s, &why) && b == -7 && s == -9 && why && *why;
}

static void check_text() {
    char buf[gol::kRuleFormatLen + 1];
    const char* why = nullptr;
    for (int birth = 0; birth <= gol::kRuleMaskMax; birth++)
        for (int survive = 0; survive <= gol::kRuleMaskMax; survive++) {
            std::memset(buf, 'x', sizeof buf);
            if (!gol::rule_format(birth, survive, buf, gol::kRuleFormatLen, &why) || buf[gol::kRuleFormatLen] != 'x' ||
                std::strlen(buf) != (size_t)(3 + __builtin_popcount(birth) + __builtin_popcount(survive)) ||
                !parses_to(buf, birth, survive))
                CHECK(!"format then parse is the identity");
        }
    CHECK(gol::rule_format(0x008, 0x00C, buf, 22, &why) && std::string(buf) == "B3/S23");
    CHECK(gol::rule_format(0x1FF, 0x1FF, buf, 22, &why) && std::string(buf) == "B012345678/S012345678");
    CHECK(gol::rule_format(0, 0, buf, 22, &why) && std::string(buf) == "B/S");
    std::strcpy(buf, "untouched");
    CHECK(!gol::rule_format(0x200, 0, buf, 22, &why) && !gol::rule_format(0, 0x200, buf, 22, &why));
    CHECK(!gol::rule_format(-1, 0, buf, 22, &why) && !gol::rule_format(0, -1, buf, 22, &why));
    CHECK(!gol::rule_format(8, 12, buf, 21, &why) && !gol::rule_format(8, 12, nullptr, 22, &why));
    CHECK(!gol::rule_format(0, 0, buf, 21, &why));  // the length is the worst case's, whatever the rule
    CHECK(std::string(buf) == "untouched");

    // the three spellings, letter case, blanks around, digits in any order
    const struct {
        int birth, survive;
        const char* forms[6];
    } same[] = {
        {0x008, 0x00C, {"B3/S23", "S23/B3", "23/3", "b3/s23", "  B3/S32\t", " 32/3 "}},
        {0x048, 0x00C, {"B36/S23", "S23/B36", "23/36", "s32/b63", "B63/s23", "\t23/63"}},
        {0x004, 0x000, {"B2/S", "S/B2", "/2", "b2/s", " B2/S ", "s/b2"}},
        {0x1C8, 0x1D8, {"B3678/S34678", "S34678/B3678", "34678/3678", "B8763/S87643", "s34678/b3678", "87643/8763"}},
        {0x000, 0x000, {"B/S", "S/B", "/", "b/s", " / ", "s/B"}},
        {0x1FF, 0x1FF, {"B012345678/S012345678", "S012345678/B012345678", "012345678/012345678", "b876543210/s012345678",
                        " B012345678/S012345678 ", "876543210/876543210"}},
        {0x001, 0x100, {"B0/S8", "S8/B0", "8/0", "b0/s8", "B0/S8  ", "  8/0"}},
    };
    for (const auto& r : same)
        for (const char* f : r.forms) CHECK(parses_to(f, r.birth, r.survive));
    CHECK(parses_to("B3/S23                         ", 8, 12));  // 31 characters

    const char* malformed[] = {
        "", " ", "\t  ", "B9/S23", "B3/S29", "9/3", "B33/S23", "B3/S232", "22/3", "B3S23", "B3", "S23", "23", "3",
        "B3/S23/3", "23/3/3", "B3/S23/", "//", "B3/S23x", "xB3/S23", "B3-S23", "B3\\S23", "B3 /S23", "B 3/S23", "B3/ S23",
        "B3/S2 3", "B3/B23", "S3/S23", "B3/23", "23/B3", "3/S23", "BB3/S23", "B3/SS23", "B3/S23\n", "B-3/S23", "B+3/S23",
        "B3.0/S23", "B3/S23 B3/S23", "B3/S23                          ",  // 32 characters
        "B012345678/S012345678/0123456789012345678901234567890123456789",
    };
    for (const char* t : malformed) CHECK(refused(t));
    CHECK(refused(nullptr));
    int b = 5, s = 6;
    const char* w = nullptr;
    CHECK(!gol::rule_parse("B3/S23", nullptr, &s, &w) && !gol::rule_parse("B3/S23", &b, nullptr, &w) && s == 6 && b == 5);
    CHECK(gol::rule_parse("B3/S23", &b, &s, nullptr) && b == 8 && s == 12);   // why may be null
    CHECK(!gol::rule_parse("B9/S23", &b, &s, nullptr) && b == 8 && s == 12);
    // a text that ends right at the buffer's end: the parser reads no further than the NUL (address sanitizer)
    char* exact = new char[7];
    std::memcpy(exact, "B3/S23", 7);
    CHECK(parses_to(exact, 8, 12));
    delete[] exact;
    char* unterminated = new char[32];
    std::memset(unterminated, '1', 32);  // 32 characters and no NUL within them: refused without reading a 33rd
    CHECK(refused(unterminated));
    delete[] unterminated;
}

// neighbourhood v (9 bits: bit 3 r + k = row r (0 above, 1 the cell's, 2 below), column k (0 west, 1 centre, 2 east))
// sits at bit v & 31 of word v >> 5
static uint32_t in[7][16];  // sP, cP, sC, cC, sN, cN, alive
static int cell_alive[512], cell_n[512];

static void make_inputs() {
    for (int v = 0; v < 512; v++) {
        for (int r = 0; r < 3; r++) {
            const int sum = (v >> (3 * r) & 1) + (v >> (3 * r + 1) & 1) + (v >> (3 * r + 2) & 1);
            in[2 * r][v >> 5] |= (uint32_t)(sum & 1) << (v & 31);
            in[2 * r + 1][v >> 5] |= (uint32_t)(sum >> 1) << (v & 31);
        }
        cell_alive[v] = v >> 4 & 1;
        cell_n[v] = __builtin_popcount(v) - cell_alive[v];
        in[6][v >> 5] |= (uint32_t)cell_alive[v] << (v & 31);
    }
}

static void check_evaluator() {
    make_inputs();
    long words = 0;
    for (int birth = 0; birth <= gol::kRuleMaskMax; birth++)
        for (int survive = 0; survive <= gol::kRuleMaskMax; survive++) {
            const uint32_t rule = gol::rule_pack(birth, survive);
            for (int k = 0; k < 16; k++) {
                uint32_t want = 0;
                for (int b = 0; b < 32; b++) {
                    const int v = 32 * k + b;
                    want |= (uint32_t)gol::rule_next_cell(cell_alive[v], cell_n[v], birth, survive) << b;
                }
                const uint32_t got = gol::rule_next(in[0][k], in[1][k], in[2][k], in[3][k], in[4][k], in[5][k], in[6][k], rule);
                words++;
                if (got != want) CHECK(!"rule_next differs from the scalar definition");
            }
        }
    CHECK(words == 16L << 18);
    // four words of a row at once (the kernels' form) agree with one at a time
    for (uint32_t rule : {gol::kRuleLifePacked, gol::rule_pack(0x1C8, 0x1D8), gol::rule_pack(0x1FF, 0x1FF), gol::rule_pack(1, 0x180)})
        for (int k = 0; k < 16; k += 4) {
            uint32_t a[7][4], out[4];
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 4; j++) a[i][j] = in[i][k + j];
            gol::rule_next_row<4>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], rule, out);
            for (int j = 0; j < 4; j++)
                CHECK(out[j] == gol::rule_next(in[0][k + j], in[1][k + j], in[2][k + j], in[3][k + j], in[4][k + j],
                                               in[5][k + j], in[6][k + j], rule));
        }
    // B3/S23: the table evaluator is life_next
    CHECK(gol::kRuleLifePacked == gol::rule_pack(gol::kRuleLifeBirth, gol::kRuleLifeSurvive));
    for (int k = 0; k < 16; k++)
        CHECK(gol::rule_next(in[0][k], in[1][k], in[2][k], in[3][k], in[4][k], in[5][k], in[6][k], gol::kRuleLifePacked) ==
              gol::life_next(in[0][k], in[1][k], in[2][k], in[3][k], in[4][k], in[5][k], in[6][k]));
    std::printf("rule evaluator: %ld words\n", words);
}

int main() {
    check_text();
    check_evaluator();
    if (bad) {
        std::printf("%ld failures\n", bad);
        return 1;
    }
    std::printf("rules ok: 262144 rules, 512 neighbourhoods\n");
    return 0;
}
