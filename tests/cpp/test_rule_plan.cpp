// test_rule_plan.cpp -- the plan of the rule-generic streaming pass (csrc/gol_rule_plan.h) walked on the host, alone,
// under the address and undefined-behaviour sanitizers (tests/test_rule_plan_host.py).  For rows of 1..200 blocks,
// heights 3..100, K in {1, 2, 4, 8}, both boundaries and forced segment rows in {0, 1, 5, 17}:
//   - every (row, block) of the board is stored by exactly one (wave, lane);
//   - every row and block index any lane loads lies inside the buffer -- after the modulo on a torus -- or is flagged
//     not loaded (bounded boards, steps past the stream), and the kernel's running row index (incremented and wrapped,
//     gol_rule_step.hip load_row) is the plan's at every step, the prefetch past the last trip included;
//   - a stored output depends on loaded rows only: the stream covers K rows above and below the stored rows, and on a
//     torus the loaded row is the true row modulo H;
//   - the wave count is nstrips * nsegs, and the grid the launcher uses covers it.
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

int main() {
    const int ks[] = {1, 2, 4, 8};
    const int64_t segs[] = {0, 1, 5, 17};
    const int64_t targets[] = {1, 64, 2048};
    long long cases = 0, waves = 0;
    char ctx[160];
    for (int64_t nb = 1; nb <= 200; nb++)
        for (int64_t H = 3; H <= 100; H++)
            for (int K : ks)
                for (int bounded = 0; bounded < 2; bounded++)
                    for (int64_t seg_opt : segs) {
                        const int64_t target = targets[(nb + H + K) % 3];
                        const RulePlan p = rule_plan(nb, H, K, bounded != 0, seg_opt, target);
                        std::snprintf(ctx, sizeof ctx, "nblocks %lld H %lld K %d bounded %d seg_opt %lld target %lld",
                                      (long long)nb, (long long)H, K, bounded, (long long)seg_opt, (long long)target);
                        cases++;
                        CHECK(p.nwaves == p.nstrips * p.nsegs && p.nwaves >= 1);
                        CHECK(p.seg >= 1 && p.seg <= H);
                        if (seg_opt > 0) CHECK(p.seg == (seg_opt < H ? seg_opt : H));
                        CHECK(rule_stream_grid(p) * kRuleWavesPerBlock >= p.nwaves);
                        CHECK((rule_stream_grid(p) - 1) * kRuleWavesPerBlock < p.nwaves);
                        std::vector<int> stored((size_t)(H * nb), 0);
                        // a wave's blocks depend on its strip alone and its rows on its segment alone (checked below on
                        // every wave's RuleWave): the lanes are walked once per strip, the steps once per segment
                        std::vector<std::vector<int64_t>> strip_stores((size_t)p.nstrips), seg_rows((size_t)p.nsegs);
                        for (int64_t wv = 0; wv < p.nwaves; wv++) {
                            const RuleWave w = rule_wave(p, wv);
                            waves++;
                            CHECK(w.r0 >= 0 && w.r0 < w.r1 && w.r1 <= H);
                            CHECK(w.steps == w.r1 - w.r0 + 2 * K);
                            CHECK(w.trips * kRuleTripRows >= w.steps && (w.trips - 1) * kRuleTripRows < w.steps);
                            CHECK(w.strip >= 0 && w.strip < p.nstrips && w.segment >= 0 && w.segment < p.nsegs);
                            CHECK(wv == w.segment * p.nstrips + w.strip);
                            CHECK(w.first_block == w.strip * kRuleStored - 1 && w.r0 == w.segment * p.seg);
                            if (w.strip >= p.nstrips || w.segment >= p.nsegs || w.strip < 0 || w.segment < 0) continue;
                            // blocks
                            int64_t lane_block[kRuleLanes];
                            bool lane_loads[kRuleLanes];
                            std::vector<int64_t>& stores = strip_stores[(size_t)w.strip];  // the blocks this wave stores
                            std::vector<int64_t>& rows = seg_rows[(size_t)w.segment];      // ... and the rows
                            for (int lane = 0; w.segment == 0 && lane < kRuleLanes; lane++) {
                                lane_loads[lane] = rule_lane_load(p, w, lane, &lane_block[lane]);
                                if (lane_loads[lane]) CHECK(lane_block[lane] >= 0 && lane_block[lane] < nb);
                                if (!bounded) {
                                    CHECK(lane_loads[lane]);
                                    CHECK((lane_block[lane] - (w.first_block + lane)) % nb == 0);  // the true block mod nb
                                } else {
                                    const int64_t raw = w.first_block + lane;
                                    CHECK(lane_loads[lane] == (raw >= 0 && raw < nb));
                                }
                                int64_t sb;
                                if (rule_lane_store(p, w, lane, &sb)) {
                                    CHECK(lane >= 1 && lane <= kRuleStored);  // both neighbours' lanes exist
                                    CHECK(sb >= 0 && sb < nb && sb == w.first_block + lane);
                                    CHECK(lane_loads[lane] && lane_block[lane] == sb);
                                    stores.push_back(sb);
                                }
                            }
                            // rows: the plan's answer, and the kernel's running index (load_row)
                            int64_t run = bounded ? w.r0 - K : rule_mod(w.r0 - K, H);
                            const int64_t tmax = (w.trips + 1) * kRuleTripRows;  // the prefetch past the last trip
                            for (int64_t t = 0; w.strip == 0 && t < tmax; t++) {
                                int64_t row;
                                const bool ld = rule_step_load(p, w, t, &row);
                                const bool kernel_ld = t < w.steps && (!bounded || (run >= 0 && run < H));
                                CHECK(ld == kernel_ld);
                                if (ld) {
                                    CHECK(row >= 0 && row < H && row == run);
                                    CHECK((row - (w.r0 - K + t)) % H == 0);
                                }
                                if (t >= w.steps) CHECK(!ld);
                                if (!bounded && t < w.steps) CHECK(ld);
                                run++;
                                if (!bounded && run == H) run = 0;
                                int64_t srow;
                                if (rule_step_store(p, w, t, &srow)) {
                                    CHECK(t < w.trips * kRuleTripRows && t >= 2 * K && t < w.steps);
                                    CHECK(srow >= w.r0 && srow < w.r1);
                                    // the rows srow - K .. srow + K were steps t - 2 K .. t: all inside the stream
                                    CHECK(srow + K == w.r0 - K + t);
                                    rows.push_back(srow);
                                }
                            }
                            for (int64_t srow : rows)
                                for (int64_t sb : stores) stored[(size_t)(srow * nb + sb)]++;
                        }
                        long long bad = 0;
                        for (int v : stored) bad += v != 1;
                        CHECK(bad == 0);
                    }
    std::printf("rule plan: %lld cases, %lld waves\n", cases, waves);
    if (g_fail) {
        std::printf("%lld failures\n", g_fail);
        return 1;
    }
    std::printf("rule plan ok\n");
    return 0;
}
