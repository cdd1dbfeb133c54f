// test_ragged_rule_plan.cpp -- the ragged rows of the rule-generic and multi-plane streaming passes (csrc/gol_rule_plan.h
// "Ragged rows") walked on the host, alone, under the address and undefined-behaviour sanitizers
// (tests/test_ragged_rule_plan_host.py).  For every width 64..4100 that is no multiple of 32, heights {3, 7, 40}, K in
// {1, 2, 4, 8}, both boundaries and segment rows {planned, 5}, on a row of known bits in whole words with zero pads (a
// heap row of exactly nw words: a read outside it is the sanitizer's):
//   - torus: the word every lane of every strip assembles through rule_ragged_window / rule_ragged_load -- the
//     functions the kernels call -- is cell[(p + b) mod W] bit for bit, p = 32 (62 strip - 1 + lane); every word index
//     read lies in [0, nw); a plain lane's word is the row's word as it stands; adjacent lanes are adjacent on the ring;
//   - bounded: the word a lane loads, ANDed with its level mask, is the row's cells with zero outside [0, W), and the
//     level mask is exactly the lane's cells inside the row;
//   - every (row, word) is stored by exactly one (wave, lane), a storing lane's window starts at cell 32 word with no
//     shift, its store mask is the real cells of that word, and exactly one lane of a row's storing lanes is partial.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../gameoflifewithactors_amd/csrc/gol_rule_plan.h"

using namespace gol;

static long long g_fail = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            if (g_fail++ < 20) std::printf("FAIL %s (line %d): %s\n", #c, __LINE__, ctx); \
        }                                                                             \
    } while (0)

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

int main() {
    const int ks[] = {1, 2, 4, 8};
    const int64_t heights[] = {3, 7, 40};
    const int64_t segs[] = {0, 5};
    const int64_t targets[] = {1, 64, 2048};
    long long cases = 0, windows = 0, shifted = 0;
    char ctx[160];
    for (int64_t W = 64; W <= 4100; W++) {
        if (W % 32 == 0) continue;
        std::snprintf(ctx, sizeof ctx, "W %lld", (long long)W);
        CHECK(rule_ragged_ok(W));
        const int64_t nw = rule_ragged_words(W);
        CHECK(nw == (W + 31) / 32 && nw * 32 > W && (nw - 1) * 32 < W);
        // the row: known cells, whole words, zero pads
        std::vector<uint8_t> cell((size_t)W);
        std::vector<uint32_t> row((size_t)nw, 0u);
        for (int64_t x = 0; x < W; x++) {
            cell[(size_t)x] = (uint8_t)(mix((uint64_t)(W * 8191 + x)) & 1);
            row[(size_t)(x / 32)] |= (uint32_t)cell[(size_t)x] << (x % 32);
        }
        cell[0] = 1, row[0] |= 1u;  // both ends alive: a missed or doubled seam cell shows
        cell[(size_t)(W - 1)] = 1, row[(size_t)(nw - 1)] |= 1u << ((W - 1) % 32);
        const uint32_t tail = rule_ragged_tail_mask(W);
        CHECK(tail == (uint32_t)((1ull << (W % 32)) - 1) && (row[(size_t)(nw - 1)] & ~tail) == 0);
        for (int64_t H : heights)
            for (int K : ks)
                for (int bounded = 0; bounded < 2; bounded++)
                    for (int64_t seg_opt : segs) {
                        const int64_t target = targets[(W + H + K) % 3];
                        const RulePlan p = rule_plan(nw, H, K, bounded != 0, seg_opt, target);
                        std::snprintf(ctx, sizeof ctx, "W %lld H %lld K %d bounded %d seg_opt %lld target %lld",
                                      (long long)W, (long long)H, K, bounded, (long long)seg_opt, (long long)target);
                        cases++;
                        CHECK(p.nblocks == nw && p.nwaves == p.nstrips * p.nsegs);
                        std::vector<int> stored((size_t)(H * nw), 0);
                        for (int64_t wv = 0; wv < p.nwaves; wv++) {
                            const RuleWave w = rule_wave(p, wv);
                            uint32_t word[kRuleLanes];
                            int partial_stores = 0;
                            // a lane's window, masks and blocks depend on its strip alone (first_block): the bits are
                            // walked on the first segment's waves, the stores counted on every wave
                            if (w.segment > 0) {
                                for (int lane = 0; lane < kRuleLanes; lane++) {
                                    int64_t sb;
                                    if (!rule_lane_store(p, w, lane, &sb)) continue;
                                    for (int64_t t = 0; t < w.trips * kRuleTripRows; t++) {
                                        int64_t srow;
                                        if (rule_step_store(p, w, t, &srow)) stored[(size_t)(srow * nw + sb)]++;
                                    }
                                }
                                continue;
                            }
                            for (int lane = 0; lane < kRuleLanes; lane++) {
                                const int64_t pos = 32 * (w.first_block + lane);  // the lane's ring position
                                int64_t blk;
                                const bool loads = rule_lane_load(p, w, lane, &blk);
                                if (!bounded) {
                                    const RaggedWindow g = rule_ragged_window(w, lane, W);
                                    windows++;
                                    shifted += !rule_ragged_plain(g);
                                    CHECK(g.word >= 0 && g.word < nw && g.shift >= 0 && g.shift < 32);
                                    CHECK(g.seam >= 1 && g.seam <= 32);
                                    if (g.second) CHECK(g.word + 1 < nw && g.shift > 0);
                                    CHECK(g.word * 32 + g.shift == rule_mod(pos, W));
                                    word[lane] = rule_ragged_load(row.data(), g);
                                    uint32_t want = 0;
                                    for (int b = 0; b < 32; b++)
                                        want |= (uint32_t)cell[(size_t)rule_mod(pos + b, W)] << b;
                                    CHECK(word[lane] == want);
                                    if (rule_ragged_plain(g)) CHECK(word[lane] == row[(size_t)g.word] && g.word < nw - 1);
                                    // the lanes the aligned arithmetic would serve are plain: inside the row, whole words
                                    if (pos >= 0 && pos + 32 <= W) CHECK(rule_ragged_plain(g) && g.word == pos / 32);
                                } else {
                                    const uint32_t m = rule_ragged_level_mask(p, w, lane, W);
                                    uint32_t want = 0, inside = 0;
                                    for (int b = 0; b < 32; b++) {
                                        const int64_t x = pos + b;
                                        if (x < 0 || x >= W) continue;
                                        inside |= 1u << b;
                                        want |= (uint32_t)cell[(size_t)x] << b;
                                    }
                                    CHECK(m == inside);
                                    CHECK(loads == (pos >= 0 && pos < W));
                                    if (loads) CHECK(blk >= 0 && blk < nw && blk == w.first_block + lane);
                                    word[lane] = loads ? row[(size_t)blk] : 0u;
                                    CHECK((word[lane] & m) == want && word[lane] == want);  // (pads are zero in memory too)
                                }
                                CHECK(rule_ragged_partial(p, w, lane) == (w.first_block + lane == nw - 1));
                                int64_t sb;
                                if (rule_lane_store(p, w, lane, &sb)) {
                                    CHECK(lane >= 1 && lane <= kRuleStored && sb >= 0 && sb < nw && sb * 32 == pos);
                                    const uint32_t sm = rule_ragged_store_mask(p, w, lane, W);
                                    uint32_t real = 0;
                                    for (int b = 0; b < 32; b++) real |= (uint32_t)(sb * 32 + b < W) << b;
                                    CHECK(sm == real);
                                    CHECK((word[lane] & sm) == row[(size_t)sb]);  // a pass of zero generations is the row
                                    partial_stores += rule_ragged_partial(p, w, lane);
                                    for (int64_t t = 0; t < w.trips * kRuleTripRows; t++) {
                                        int64_t srow;
                                        if (rule_step_store(p, w, t, &srow)) stored[(size_t)(srow * nw + sb)]++;
                                    }
                                }
                            }
                            // the partial word's lane is stored by the strip that holds it, with a lane to its right
                            CHECK(partial_stores == (w.strip == p.nstrips - 1 ? 1 : 0));
                        }
                        long long bad = 0;
                        for (int v : stored) bad += v != 1;
                        CHECK(bad == 0);
                    }
    }
    std::printf("ragged rule plan: %lld cases, %lld torus windows, %lld of them assembled\n", cases, windows, shifted);
    if (g_fail) {
        std::printf("%lld failures\n", g_fail);
        return 1;
    }
    std::printf("ragged rule plan ok\n");
    return 0;
}
