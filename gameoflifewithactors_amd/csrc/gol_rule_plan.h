// gol_rule_plan.h -- the segment and strip plan of the rule-generic streaming pass (gol_rule_step.hip):
// which wave stores which rows and blocks of a packed board, how many rows and trips it streams, and which row and
// block every lane loads.  Plain arithmetic: the launcher plans with it, the kernel derives its wave's geometry from the
// same functions, and tests/cpp/test_rule_plan.cpp walks it alone under the sanitizers.
//
//   columns  a row is nblocks interleaved blocks (gol_layout.h).  Strip s stores blocks [62 s, 62 s + 62) of it; its
//            wave's lane i holds block 62 s - 1 + i, so lanes 0 and 63 are halo and lanes 1..62 store.
//   rows     segment g stores rows [g seg, g seg + seg) (the last one to H).  Its wave streams the rows from K above
//            the first to K below the last, seg + 2 K of them, three per loop trip; step t of the stream loads row
//            r0 - K + t, and the last level's output at step t is row r0 - 2 K + t.
//   torus    block and row indices are taken modulo nblocks and H (a true modulo: a 3-row board at K = 8 wraps several
//            times, a row of fewer than 62 blocks repeats across the lanes).
//   bounded  blocks and rows outside the board are not loaded (they read as zero, and are forced dead at every level).
//   Steps past the stream (the last trip's tail) and the prefetch past the last trip load nothing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GOL_PLAN_HD __host__ __device__ __forceinline__
#else
#define GOL_PLAN_HD static inline
#endif

namespace gol {

static constexpr int kRuleLanes = 64;
static constexpr int kRuleStored = kRuleLanes - 2;  // blocks a wave stores per row
static constexpr int kRuleTripRows = 3;             // rows per loop trip (the 3-row window rotates once per trip)
static constexpr int kRuleWavesPerBlock = 4;

struct RulePlan {
    int64_t nblocks;  // blocks per row
    int64_t H;        // rows of the board
    int64_t seg;      // rows stored per segment (the last may be shorter)
    int64_t nstrips, nsegs;
    int64_t nwaves;   // nstrips * nsegs
    int32_t K;        // generations of the pass
    int32_t bounded;
};

// What one wave does.
struct RuleWave {
    int64_t strip, segment;
    int64_t first_block;  // lane 0's block, 62 strip - 1 (before the modulo)
    int64_t r0, r1;       // rows [r0, r1) stored
    int64_t steps;        // rows streamed, r1 - r0 + 2 K
    int64_t trips;        // loop trips, ceil(steps / 3)
};

GOL_PLAN_HD int64_t rule_mod(int64_t a, int64_t n) {  // a mod n in [0, n), whatever a's sign
    const int64_t r = a % n;
    return r < 0 ? r + n : r;
}

// seg_opt: 0 = planned (about target_waves waves, segments of at least 2 K rows: at most half of what a wave streams is
// recomputed), > 0 = that many rows per segment.
GOL_PLAN_HD RulePlan rule_plan(int64_t nblocks, int64_t H, int K, bool bounded, int64_t seg_opt, int64_t target_waves) {
    RulePlan p;
    p.nblocks = nblocks;
    p.H = H;
    p.K = K;
    p.bounded = bounded ? 1 : 0;
    p.nstrips = (nblocks + kRuleStored - 1) / kRuleStored;
    int64_t seg;
    if (seg_opt > 0) {
        seg = seg_opt;
    } else {
        int64_t want = target_waves / p.nstrips;
        if (want < 1) want = 1;
        seg = (H + want - 1) / want;
        if (seg < 2 * (int64_t)K) seg = 2 * (int64_t)K;
    }
    if (seg > H) seg = H;
    p.seg = seg;
    p.nsegs = (H + seg - 1) / seg;
    p.nwaves = p.nstrips * p.nsegs;
    return p;
}

// Waves that share rows are neighbours: wave = segment * nstrips + strip.
GOL_PLAN_HD RuleWave rule_wave(const RulePlan& p, int64_t wave) {
    RuleWave w;
    w.segment = wave / p.nstrips;
    w.strip = wave - w.segment * p.nstrips;
    w.first_block = w.strip * kRuleStored - 1;
    w.r0 = w.segment * p.seg;
    w.r1 = w.r0 + p.seg < p.H ? w.r0 + p.seg : p.H;
    w.steps = w.r1 - w.r0 + 2 * (int64_t)p.K;
    w.trips = (w.steps + kRuleTripRows - 1) / kRuleTripRows;
    return w;
}

// The block lane `lane` loads: false = nothing (it reads as zero), else *block in [0, nblocks).
GOL_PLAN_HD bool rule_lane_load(const RulePlan& p, const RuleWave& w, int lane, int64_t* block) {
    const int64_t raw = w.first_block + lane;
    if (p.bounded) {
        *block = raw;
        return raw >= 0 && raw < p.nblocks;
    }
    *block = rule_mod(raw, p.nblocks);
    return true;
}

// The block lane `lane` stores (rows [r0, r1)): false = none.
GOL_PLAN_HD bool rule_lane_store(const RulePlan& p, const RuleWave& w, int lane, int64_t* block) {
    *block = w.first_block + lane;
    return lane >= 1 && lane <= kRuleStored && *block < p.nblocks;
}

// The row step t (0 .. 3 trips - 1) loads: false = nothing, else *row in [0, H).
GOL_PLAN_HD bool rule_step_load(const RulePlan& p, const RuleWave& w, int64_t t, int64_t* row) {
    const int64_t raw = w.r0 - p.K + t;
    *row = raw;
    if (t >= w.steps) return false;  // past the stream
    if (p.bounded) return raw >= 0 && raw < p.H;
    *row = rule_mod(raw, p.H);
    return true;
}

// The row the last level's output of step t is stored to: false = not stored.
GOL_PLAN_HD bool rule_step_store(const RulePlan& p, const RuleWave& w, int64_t t, int64_t* row) {
    *row = w.r0 - 2 * (int64_t)p.K + t;
    return *row >= w.r0 && *row < w.r1;
}

GOL_PLAN_HD int64_t rule_stream_grid(const RulePlan& p) {  // workgroups of kRuleWavesPerBlock waves
    return (p.nwaves + kRuleWavesPerBlock - 1) / kRuleWavesPerBlock;
}

// ---- Ragged rows: a board of W cells per row, W >= 64 and not a multiple of 32, as rows of
// nw = ceil(W / 32) consecutive words (blocks of one word), bit b of word j = cell 32 j + b, the W % 32 real cells of
// the last word in its low bits and its pad bits ZERO.  The plan is rule_plan(nw, ...), the strips, segments, rows and
// stored blocks are the functions above, and a lane is 32 consecutive cells of the ring of W cells at ring position
// 32 (first_block + lane):
//   torus    the lane's word is ring cells [q, q + 32), q = position mod W.  Where q is a multiple of 32 and the window
//            ends inside the row that is word q / 32 as it stands; every other lane -- the halo lane left of word 0,
//            the lane of the partial last word and all lanes to its right -- assembles it from up to three words: word
//            q / 32 and the next shifted down by q % 32, and, where the window crosses the row's end after n < 32
//            cells, word 0 shifted up by n (W >= 64: the window crosses the end at most once, and what follows it lies
//            in word 0).  The zero pad bits are what lets the three parts be ORed together.
//   bounded  a lane inside the row loads its word, the others nothing (rule_lane_load); the lane of the partial word
//            keeps only its real cells alive at every level (rule_ragged_level_mask).
//   stores   rule_lane_store's lanes; the lane of the partial word stores its real cells only (rule_ragged_store_mask),
//            so pad bits stay zero from pass to pass.
static constexpr int64_t kRuleRaggedMinWidth = 64;

GOL_PLAN_HD int64_t rule_ragged_words(int64_t W) { return (W + 31) / 32; }

GOL_PLAN_HD bool rule_ragged_ok(int64_t W) { return W >= kRuleRaggedMinWidth && W % 32 != 0; }

GOL_PLAN_HD uint32_t rule_ragged_tail_mask(int64_t W) { return (1u << (uint32_t)(W % 32)) - 1u; }  // W % 32 != 0

// The window of a torus lane: word `word`, with `second` also word + 1 (both in [0, nw)), and with seam < 32 word 0.
struct RaggedWindow {
    int64_t word;
    int32_t shift;   // 0..31: the window starts at bit `shift` of `word`
    int32_t second;  // 1: the window goes on in word + 1 (shift > 0, and `word` is not the row's last)
    int32_t seam;    // cells of the window before the row's end, 1..31; 32 = the window does not cross it
};

GOL_PLAN_HD RaggedWindow rule_ragged_window(const RuleWave& w, int lane, int64_t W) {
    const int64_t q = rule_mod(32 * (w.first_block + lane), W);
    RaggedWindow g;
    g.word = q / 32;
    g.shift = (int32_t)(q % 32);
    g.second = g.shift > 0 && g.word + 1 < rule_ragged_words(W);
    g.seam = W - q < 32 ? (int32_t)(W - q) : 32;
    return g;
}
GOL_PLAN_HD bool rule_ragged_plain(const RaggedWindow& g) { return g.shift == 0 && g.seam == 32; }

// The lane's word from the words it read: a = row[word], b = row[word + 1] (if second, else anything), c = row[0] (if
// seam < 32, else anything).
GOL_PLAN_HD uint32_t rule_ragged_assemble(const RaggedWindow& g, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t v = a >> (uint32_t)g.shift;
    if (g.second) v |= b << (32u - (uint32_t)g.shift);
    if (g.seam < 32) v |= c << (uint32_t)g.seam;
    return v;
}

// ... read from the row (nw words) itself
GOL_PLAN_HD uint32_t rule_ragged_load(const uint32_t* row, const RaggedWindow& g) {
    const uint32_t a = row[g.word];
    const uint32_t b = g.second ? row[g.word + 1] : 0u;
    const uint32_t c = g.seam < 32 ? row[0] : 0u;
    return rule_ragged_assemble(g, a, b, c);
}

// The lane that holds the row's partial last word (as a block of the row, before any modulo)
GOL_PLAN_HD bool rule_ragged_partial(const RulePlan& p, const RuleWave& w, int lane) {
    return w.first_block + lane == p.nblocks - 1;
}

// What a storing lane (rule_lane_store) writes of its word: the real cells
GOL_PLAN_HD uint32_t rule_ragged_store_mask(const RulePlan& p, const RuleWave& w, int lane, int64_t W) {
    return rule_ragged_partial(p, w, lane) ? rule_ragged_tail_mask(W) : 0xffffffffu;
}

// Bounded boards: the cells of the lane's word that may live, ANDed into every level's output (in rows inside the
// board): none outside the row, the real cells of the partial word, else all.
GOL_PLAN_HD uint32_t rule_ragged_level_mask(const RulePlan& p, const RuleWave& w, int lane, int64_t W) {
    const int64_t raw = w.first_block + lane;
    if (raw < 0 || raw >= p.nblocks) return 0u;
    return raw == p.nblocks - 1 ? rule_ragged_tail_mask(W) : 0xffffffffu;
}

}  // namespace gol
