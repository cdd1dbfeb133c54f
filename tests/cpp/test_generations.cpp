// test_generations.cpp -- csrc/gol_generations.h on the CPU, under the address and undefined-behaviour sanitizers
// (tests/test_generations_host.py builds and runs it): the bit-sliced transition (rule_next_row + gen_decay on the
// bit-plane encoding) against the scalar definition gen_next_cell, and the three-field parser and formatter.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../gameoflifewithactors_amd/csrc/gol_generations.h"

using namespace gol;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            if (++failures > 20) exit(1);                          \
        }                                                          \
    } while (0)

// 32 cells of one word: cell b is in state st[b] with nb[b] neighbours in state 1.  The neighbours are laid out as the
// three row sums rule_next_row takes: row above a + row below c horizontal sums (each 0..3), centre row sum includes the
// centre cell.  Returns the next states through the planes.
template <int P>
static void run_word(const int (&st)[32], const int (&nb)[32], int birth, int survive, int nstates, int (&out)[32]) {
    uint32_t sP[1] = {0}, cP[1] = {0}, sC[1] = {0}, cC[1] = {0}, sN[1] = {0}, cN[1] = {0}, alive[1] = {0};
    uint32_t d[P];
    for (int k = 0; k < P; k++) d[k] = 0;
    for (int b = 0; b < 32; b++) {
        int n = nb[b];
        const int up = n > 3 ? 3 : n;
        n -= up;
        const int dn = n > 3 ? 3 : n;
        n -= dn;  // 0..2 beside the centre
        const int mid = n + (st[b] == 1);
        sP[0] |= (uint32_t)(up & 1) << b, cP[0] |= (uint32_t)(up >> 1) << b;
        sN[0] |= (uint32_t)(dn & 1) << b, cN[0] |= (uint32_t)(dn >> 1) << b;
        sC[0] |= (uint32_t)(mid & 1) << b, cC[0] |= (uint32_t)(mid >> 1) << b;
        alive[0] |= (uint32_t)(st[b] == 1) << b;
        const int dd = st[b] >= 2 ? st[b] - 1 : 0;
        for (int k = 0; k < P; k++) d[k] |= (uint32_t)(dd >> k & 1) << b;
    }
    uint32_t v[1];
    rule_next_row<1>(sP, cP, sC, cC, sN, cN, alive, rule_pack(birth, survive), v);
    const uint32_t a = gen_decay<P>(alive[0], v[0], d, gen_masks(nstates));
    for (int b = 0; b < 32; b++) {
        int dd = 0;
        for (int k = 0; k < P; k++) dd |= (int)(d[k] >> b & 1) << k;
        const int al = (int)(a >> b & 1);
        CHECK(!(al && dd));  // the planes stay exclusive
        out[b] = al ? 1 : dd ? dd + 1 : 0;
        for (int k = 1; k < nstates; k++) {  // and the indicator words name the state
            const uint32_t w = gen_state_word(a, [&](int q) { return d[q]; }, P, k);
            CHECK((int)(w >> b & 1) == (out[b] == k));
        }
    }
}

static void run(const int (&st)[32], const int (&nb)[32], int birth, int survive, int nstates, int (&out)[32]) {
    switch (gen_planes(nstates)) {
        case 1: return run_word<1>(st, nb, birth, survive, nstates, out);
        case 2: return run_word<2>(st, nb, birth, survive, nstates, out);
        case 3: return run_word<3>(st, nb, birth, survive, nstates, out);
    }
    // 2 states: the life-like rule itself, no plane
    for (int b = 0; b < 32; b++) out[b] = rule_next_cell(st[b], nb[b], birth, survive);
}

static long transition() {
    long words = 0;
    std::mt19937 rng(12345);
    int st[32], nb[32], out[32];
    // every nstates, every state, every n, both values of the rule bit that matters; the word's other cells mixed
    for (int C = 2; C <= 8; C++)
        for (int s = 0; s < C; s++)
            for (int n = 0; n <= 8; n++)
                for (int bit = 0; bit < 2; bit++)
                    for (int rep = 0; rep < 4; rep++) {
                        int birth = (int)(rng() & 0x1FF), survive = (int)(rng() & 0x1FF);
                        birth = (birth & ~(1 << n)) | (s == 0 ? bit << n : (int)(rng() & 1) << n);
                        survive = (survive & ~(1 << n)) | (s == 1 ? bit << n : (int)(rng() & 1) << n);
                        for (int b = 0; b < 32; b++) st[b] = (int)(rng() % (unsigned)C), nb[b] = (int)(rng() % 9);
                        const int at = (int)(rng() % 32);
                        st[at] = s, nb[at] = n;
                        run(st, nb, birth, survive, C, out);
                        for (int b = 0; b < 32; b++) CHECK(out[b] == gen_next_cell(st[b], nb[b], birth, survive, C));
                        words++;
                    }
    CHECK(gen_next_cell(1, 3, 8, 0, 2) == 0 && gen_next_cell(1, 3, 8, 0, 3) == 2 && gen_next_cell(2, 0, 0, 0, 3) == 0);
    CHECK(gen_next_cell(2, 0, 0x1FF, 0x1FF, 4) == 3 && gen_next_cell(3, 8, 0x1FF, 0x1FF, 4) == 0);
    // a few thousand random full rules
    for (int i = 0; i < 4000; i++) {
        const int C = 2 + (int)(rng() % 7), birth = (int)(rng() & 0x1FF), survive = (int)(rng() & 0x1FF);
        for (int b = 0; b < 32; b++) st[b] = (int)(rng() % (unsigned)C), nb[b] = (int)(rng() % 9);
        run(st, nb, birth, survive, C, out);
        for (int b = 0; b < 32; b++) CHECK(out[b] == gen_next_cell(st[b], nb[b], birth, survive, C));
        words++;
    }
    for (int C = 2; C <= 8; C++) CHECK(gen_planes(C) == (C == 2 ? 0 : C == 3 ? 1 : C <= 5 ? 2 : 3));
    return words;
}

static long texts() {
    long n = 0;
    std::mt19937 rng(777);
    const char* why = nullptr;
    for (int i = 0; i < 3000; i++)
        for (int C = 2; C <= 8; C++) {
            const int birth = (int)(rng() & 0x1FF), survive = (int)(rng() & 0x1FF);
            std::vector<char> heap(kGenFormatLen);  // exactly the documented length: the sanitizer guards the end
            CHECK(generations_format(birth, survive, C, heap.data(), kGenFormatLen, &why));
            int b = -1, s = -1, c = -1;
            CHECK(generations_parse(heap.data(), &b, &s, &c, &why));
            CHECK(b == birth && s == survive && c == C);
            char two[kRuleFormatLen];
            CHECK(rule_format(birth, survive, two, sizeof two, &why));
            if (C == 2)
                CHECK(strcmp(two, heap.data()) == 0);
            else
                CHECK(std::string(heap.data()) == std::string(two) + "/C" + std::to_string(C));
            n++;
        }
    {
        std::vector<char> heap(kGenFormatLen);
        CHECK(generations_format(0x1FF, 0x1FF, 8, heap.data(), kGenFormatLen, &why));
        CHECK(strlen(heap.data()) == (size_t)kGenFormatLen - 1);
        char buf[40];
        memset(buf, '?', sizeof buf);
        CHECK(!generations_format(8, 12, 3, buf, kGenFormatLen - 1, &why) && buf[0] == '?');
        CHECK(!generations_format(8, 12, 1, buf, 40, &why) && !generations_format(8, 12, 9, buf, 40, &why));
        CHECK(!generations_format(0x200, 12, 3, buf, 40, &why) && !generations_format(8, 12, 3, nullptr, 40, &why));
        for (int i = 0; i < 40; i++) CHECK(buf[i] == '?');
    }
    const char* good[] = {"B3/S23/3", "b2/s/c3", "B2/S345/G4", "S23/B3/g8", " 23/3/5\t", "B2/S/2", "/2/3", "//3"};
    const int want[][3] = {{8, 12, 3}, {4, 0, 3}, {4, 0x38, 4}, {8, 12, 8}, {8, 12, 5}, {4, 0, 2}, {4, 0, 3}, {0, 0, 3}};
    for (int i = 0; i < 8; i++) {
        int b = -1, s = -1, c = -1;
        CHECK(generations_parse(good[i], &b, &s, &c, &why));
        CHECK(b == want[i][0] && s == want[i][1] && c == want[i][2]);
    }
    int b = -1, s = -1, c = -1;
    CHECK(generations_parse("B36/S23", &b, &s, &c, &why) && b == 0x48 && s == 12 && c == 2);
    const char* bad[] = {"B3/S23/", "B3/S23/1", "B3/S23/9", "B3/S23/C", "B3/S23/C9", "B3/S23/3/4", "B3/S23/X3", "B3/S23/33",
                         "B3/S23/C 3", "B3/S23 /3", "B3/S23/ 3", "B9/S23/3", "B3S23/3", "", "B3/S23/10", "B3/S23/03",
                         "Conway"};
    for (const char* t : bad) {
        int bb = -5, ss = -6, cc = -7;
        why = nullptr;
        CHECK(!generations_parse(t, &bb, &ss, &cc, &why));
        CHECK(bb == -5 && ss == -6 && cc == -7 && why && *why);
        n++;
    }
    {  // 31 characters are taken, 32 refused
        const std::string ok = std::string("B3/S23/3") + std::string(23, ' '), lng = ok + " ";
        int bb = -5, ss = -6, cc = -7;
        CHECK(!generations_parse(lng.c_str(), &bb, &ss, &cc, &why) && bb == -5 && ss == -6 && cc == -7);
        CHECK(generations_parse(ok.c_str(), &bb, &ss, &cc, &why) && bb == 8 && ss == 12 && cc == 3);
    }
    CHECK(!generations_parse(nullptr, &b, &s, &c, &why) && !generations_parse("B3/S23", &b, &s, nullptr, &why));
    int b2 = -1, s2 = -1;
    CHECK(!rule_parse("B3/S23/3", &b2, &s2, &why) && b2 == -1 && s2 == -1);  // the two-field parser still refuses it
    return n;
}

int main() {
    const long w = transition();
    printf("generations transition: %ld words\n", w);
    const long t = texts();
    printf("generations texts: %ld\n", t);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("generations ok\n");
    return 0;
}
