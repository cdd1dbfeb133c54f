// gol_policy.cpp -- which layout and depth a new board gets, and which pass a gol_step call takes (choose_pass), with
// the measurements behind every cut-over.  Host code: it launches nothing (gol_passes.cpp runs what is chosen here).
// gol_board.h declares what the other files use.
#include "gol_board.h"
#include "gol_wave_shape.h"

namespace gol {

// Interleave for a packed board of this width (gol_layout.h).  Measured on MI355X at 65536^2
// (profiles/r1/sweep_ilv.log, w12_sweep*.log): ilv 2 with K = 12 is the fastest configuration, ilv 4 needs 240 window
// VGPRs at K = 8 (2 waves/SIMD) and wastes 1/9 of its lanes on a 65536-wide row, ilv 1 pays 4x the
// funnel shifts.  gol_create_ex takes an explicit interleave (experiments).
int pick_ilv(int64_t width) {
    if (width % 64 == 0) return 2;
    return 1;
}

// Default generations per pass for a layout (measured on MI355X, DESIGN.md "Temporal block depth").
int default_tblock(int ilv) { return ilv == 4 ? 8 : (ilv == 2 ? 12 : 32); }

// Boards below this many cells are latency-bound, not throughput-bound: too few rows per wave to fill the
// device, so a deep pass is one long serial chain per wave.  They get narrow strips (ilv 1) and a shallow
// block (K = 8): 4096^2 8.8k vs 3.8k GCUPS at the large-board default (ilv 2, K = 12), 1024^2 554 vs 240,
// 256^2 bounded 21.7 vs 13.3 (profiles/r1/small_sweep.log).
constexpr int64_t kSmallBoardCells = (int64_t)1 << 25;
// Mid-size boards (up to 2^29 cells) run one level deeper at ilv 2: 16384^2 K = 16 56.1k vs K = 12 54.1k.
constexpr int64_t kMidBoardCells = (int64_t)1 << 29;
// LDS-resident pass (gol_resident.hip) cut-overs, measured on MI355X (profiles/r1/resident_small.log):
// packed 256^2 0.91 vs 1.47 us/generation on the streaming pass, 512x256 1.23 vs 1.47, but 512^2 1.87 vs
// 1.49.  Byte boards: off by default.  The ragged boards it could still take (the single-wave pass takes
// W <= 128 and H <= 256, the reference's 100^2 board included) ran slower on it than on the per-generation
// byte step in an interleaved A/B: 129x127 3.46 vs 3.10 us/generation, 200x100 3.65 vs 3.10, 181^2 6.26 vs
// 3.15, 255x257 10.7 vs 3.1; only 255x64 was level, 3.00 vs 3.12 (profiles/r2/byte_cut_ab.log).
// The board option "resident_max_cells" still forces it (tests).
constexpr int64_t kResidentMaxCells = (int64_t)1 << 17;
constexpr int64_t kResidentBytesMaxCells = 0;

// Cooperative register-band pass (gol_coop.hip) for packed boards the single-wave pass does not take, up to this
// many cells and 8192 wide: 4096^2 0.81 vs 1.62 us/generation on the streaming pass, 2048^2 0.44 vs 1.48, 512^2
// 0.50 vs 1.49 (profiles/r2/ab_coop_xh_u.log), 8192 x 4096 1.76 vs 2.95, 8192^2 2.16 vs 4.25, 4096 x 8192 1.01
// vs 4.14 (coop_wide_u.log, coop_wide_s.log); below the LDS-resident cut-over too: 256^2 bounded 0.41 vs 0.92 on
// the LDS-resident pass, 512 x 256 0.50 vs 1.22 (cut_resident_q.log).  The board options "coop" (0 disables it:
// the LDS-resident and streaming passes then take these boards) and "coop_max_cells" move the cut-over.
const int64_t kCoopMaxCells = (int64_t)1 << 26;

// The level-pipelined pass (gol_pipe.hip): boards (or strips) of at least this many cells whose rows
// hold at least one strip of blocks of 128 cells -- 62 stored on a torus, 64 on a bounded board -- get ilv 4 and its
// depth (bounded 65536^2 in the driver's window: 124.0-124.7k GCUPS against 120.9-121.7k for the streaming pass's
// ilv 2, K = 12, profiles/r6/bounded/)
constexpr int64_t kPipeMinCells = (int64_t)1 << 30;
constexpr int kPipeK = 32;
bool pipe_shape(int64_t width, int64_t rows, int boundary) {
    return width % 128 == 0 && width / 128 >= (boundary == GOL_TORUS ? 62 : 64) && width * rows >= kPipeMinCells;
}

// Words per interleaved block of the cooperative pass for rows of `width` cells (0: it does not take them); the layout
// rule (board_ilv) and the pass choice (use_coop) both start from it.
int coop_ilv(int64_t width) { return width % 32 == 0 ? gol::coop_m(width / 32) : 0; }

// Layout and depth a new board gets when the caller leaves them at 0.  nparts: row strips (devices) of the board.
int board_ilv(int64_t width, int64_t height, int nparts, int boundary) {
    const int64_t cells = width * height;
    if (pipe_shape(width, height / nparts, boundary)) return 4;
    // single boards the cooperative pass takes: its interleave, so a block costs 2 funnel shifts instead of 2 per
    // word (a multi-GPU board never runs that pass: it keeps the streaming layout)
    const int m = coop_ilv(width);
    if (nparts == 1 && m > 1 && cells > kResidentMaxCells && cells <= kCoopMaxCells) return m;
    return cells < kSmallBoardCells ? 1 : pick_ilv(width);
}

int board_tblock(int ilv, int64_t cells, int boundary) {
    // byte boards (ragged widths): the ragged streaming pass runs ilv 1 words, as small ilv-1 boards do; one level
    // deeper above 2^27 cells (torus, per generation, K = 16 / 24: 10001^2 3.6-3.8 / 4.4-4.6 us, 16383^2 7.7-8.2 /
    // 7.0-7.2, 23171^2 12.5-12.9 / 12.0-12.3, 32767^2 23.2-23.5 / 22.3-22.4, 65535^2 84.4-85.6 / 83.7-84.1;
    // profiles/r3/ragged_stream_k_b.log, ragged_stream_k_m.log)
    if (ilv == 0) return cells < kSmallBoardCells ? 8 : (cells < ((int64_t)1 << 27) ? 16 : 24);
    if (ilv == 1 && cells < kSmallBoardCells) return 8;
    // Mid-size boards run one level deeper.  Large bounded boards ran best at K = 16 in rounds 1-2 (the masked
    // variant); since round 3's staged passes K = 12 leads there as on the torus: the whole 10k-generation job at
    // 65536^2 127.5k vs 119.2k GCUPS (profiles/r3/bench_bounded_job_d.log).  Ghost-row strips (multi-GPU) keep
    // K = 12: over a whole job 114k vs 100k GCUPS for K = 16 (profiles/r1/strip_k_ab.log).
    if (ilv == 2 && cells < kMidBoardCells) return 16;
    if (ilv == 4 && cells >= kPipeMinCells) return kPipeK;
    return default_tblock(ilv);
}

// Boards up to this many cells run every gol_step call as ONE launch of the LDS-resident kernel
// (gol_resident.hip) when the layout fits it: whole board in one workgroup's LDS, one barrier per
// generation.  The board option "resident_max_cells" overrides (0 disables; tests/test_gpu_resident.py).
int64_t resident_max_cells(const gol_board* b) {
    if (b->opt.resident_max_cells >= 0) return b->opt.resident_max_cells;
    return b->packed ? kResidentMaxCells : kResidentBytesMaxCells;
}
bool use_resident(const gol_board* b) {
    return b->W * b->H <= resident_max_cells(b) &&
           (b->packed ? b->ilv == 1 && gol::resident_packed_fits(b->W, b->H) : gol::resident_bytes_fits(b->W, b->H));
}

// Boards small enough for one wavefront's registers (gol_wave.hip: W <= 128, H <= 256) run every gol_step call
// as one single-wave launch (board option "wave_resident" = 0 disables it).
bool use_wave_resident(const gol_board* b) {
    if (!b->opt.wave_resident) return false;
    // the rule family also takes rows that do not divide into lanes; a B3/S23 board's choice is what it was
    const int rpl = b->rule_family() ? gol::wave_rule_rpl(b->W, b->H) : gol::wave_resident_rpl(b->W, b->H);
    return rpl > 0 && (!b->packed || b->ilv == 1);
}

// Generations per hand-off of the cooperative pass: the board's "coop_k" option if set, else its temporal-block
// cap, at most gol::kCoopDefaultK.
int coop_depth(const gol_board* b) {
    if (b->opt.coop_k > 0) return b->opt.coop_k;
    return b->tblock < gol::kCoopDefaultK ? b->tblock : gol::kCoopDefaultK;
}

// The rows-on-lanes band pass (gol_lanes.hip) on a packed single board, for a call of `gens` generations: the boards
// the cooperative pass would take whose width splits into windows (64 (m - 1) columns each), calls of at least two
// hand-off blocks (the pass stages the board through LDS at both ends of a launch).
// By default (option "lanes" 2) it takes the sizes where it measured faster than the cooperative pass: rows of <= 1024
// cells (profiles/r4/lanes_ab_j.log, us/generation, lanes vs cooperative: 256^2 0.35 vs 0.49, 512^2 0.37 vs 0.49, 1024 x
// 2048 0.41 vs 0.51).  Round 4 also gave it 8192-wide boards up to 4096 rows (m = 9: 8192 x 2048 1.08 vs 1.55); round
// 5's 16-byte granules took the cooperative pass there to 0.88-0.98 / 1.01-1.09 against 1.10 / 1.18 for the lanes
// (profiles/r5/coop_delay_ab_m.log, coop_errword_ab_l.log), so 2048- to 8192-wide boards are the cooperative pass's.
bool lanes_by_size(int64_t W, int64_t H) {
    (void)H;
    return W <= 1024;
}

// Its hand-off depth: the "coop_k" option if set, else up to 10 on rows of <= 1024 cells (the deepest a 32-row
// window holds beside a band of >= k rows; there the pass is hand-off bound: 256^2 bounded 0.32 vs 0.36 us/generation
// at k = 8, 512^2 0.33 vs 0.37, 1024 x 2048 0.36 vs 0.41, profiles/r4/lanes_k_o.log), else the cooperative depth.
int lanes_depth(const gol_board* b) {
    if (b->opt.coop_k > 0) return b->opt.coop_k;
    if (b->W > 1024) return coop_depth(b);
    return b->tblock_set && b->tblock < 10 ? b->tblock : 10;
}

bool use_lanes(const gol_board* b, int64_t gens) {
    if (!b->opt.lanes || !b->opt.coop || !b->packed || b->multi) return false;
    if (b->opt.lanes == 2 && !lanes_by_size(b->W, b->H)) return false;
    // every band resident at once: a tall narrow board plans more bands than the device holds
    return gens >= 2 * lanes_depth(b) && b->W * b->H <= b->opt.coop_max_cells &&
           gol::lanes_fits(b->W, b->H, lanes_depth(b), b->opt.lanes_m, b->ilv, b->boundary == GOL_BOUNDED);
}

bool use_coop(const gol_board* b) {
    if (!b->opt.coop || !b->packed) return false;
    const int cm = coop_ilv(b->W);
    int nwg = 0, B = 0, R = 0;
    return (b->ilv == 1 || b->ilv == cm) && b->W * b->H <= b->opt.coop_max_cells &&
           gol::coop_plan(b->W, b->H, coop_depth(b), &nwg, &B, &R, b->opt.coop_r) && nwg < kCoopFlagWords;
}

// Words per lane of the cooperative pass for a ragged row of nw words (rows padded to a multiple of it).
int coop_m_ragged(int64_t nw) { return nw <= 64 ? 1 : (nw <= 128 ? 2 : (nw <= 256 ? 4 : 0)); }

// Ragged byte boards (width not a multiple of 32) the single-wave pass does not take run on the cooperative pass
// through whole-word scratch rows when a call has at least this many generations: the per-generation byte step
// costs ~3.1 us per generation (profiles/r2/byte_cut_ab.log), the pack / unpack launches around the pass a few
// generations' worth.
constexpr int64_t kCoopRaggedMinGens = 16;
bool use_coop_ragged(const gol_board* b, int64_t* pitch) {
    if (!b->opt.coop || b->packed || b->W % 32 == 0) return false;
    const int64_t nw = (b->W + 31) / 32;
    const int cm = coop_m_ragged(nw);
    if (!cm || b->W * b->H > b->opt.coop_max_cells) return false;
    const int64_t nwp = (nw + cm - 1) / cm * cm;
    int nwg = 0, B = 0, R = 0;
    if (!gol::coop_plan(nwp * 32, b->H, coop_depth(b), &nwg, &B, &R, b->opt.coop_r) || nwg >= kCoopFlagWords)
        return false;
    *pitch = nwp;
    return true;
}

// Ragged byte boards the cooperative pass does not take (wider than 8192 cells or above 2^26 cells) run the
// streaming pass on whole-word scratch rows -- ceil(W / 32) words, the last one partial, the row end closed at bit
// level (gol_step.hip kRagged; bounded: the column-masked variant) -- packed once per gol_step call of at least this
// many generations; shorter calls take the per-generation byte step.
constexpr int64_t kStreamRaggedMinGens = 4;
bool use_stream_ragged(const gol_board* b) {
    if (b->packed || b->W % 32 == 0 || !b->opt.ragged_stream) return false;
    return (b->W + 31) / 32 >= 64;  // rows of at least one wave strip (the strip geometry's assumption)
}

// Ragged boards on the streaming pass run as block rows (gol_formats.hip) in the aligned layouts.  Torus: ring rows
// of ring_pitch(W) words, the board's cells at positions 64 .. 64 + W - 1 and copies of its ends around them, stepped
// by the ALIGNED torus kernel (seam strips, interleaved blocks: the headline kernel's instruction stream) with the two
// copies rewritten after every pass.  Bounded: rows of ceil(W / 64) blocks, the last one partial, on edge-fill strips
// that AND per-word column masks at every level (gol_step.hip NARROW = 2).  Layout and depth follow the aligned rules
// for a board of that many cells (board_ilv / board_tblock): ilv 2 from 2^25 cells, K = 16 below 2^29, 12 above.
// Block rows beat the ilv-1 rows from about 2^27.6 cells (profiles/r4/ragged_ab_b.log, us/generation, torus /
// bounded): 65535^2 41-43 vs 60 / 44-47 vs 52-54, 16383^2 5.2 vs 6.0 / 5.7 vs 5.6; below they lose: 8193 x 20000 5.0
// vs 4.7 / 4.9 vs 4.5, 10001^2 4.7 vs 3.6 / 4.6 vs 3.4.  Option "ragged_ring": 1 = by this size, 2 = always, 0 = never.
constexpr int64_t kRingMinCells = (int64_t)3 << 26;
bool ring_by_size(int64_t W, int64_t H) { return W * H >= kRingMinCells; }
bool use_ring(const gol_board* b) {
    return b->opt.ragged_ring == 2 || (b->opt.ragged_ring == 1 && ring_by_size(b->W, b->H));
}
// Ragged byte boards under another rule, life-like or Generations: the rule-generic and the multi-plane streaming pass
// on the same ilv-1 whole-word scratch rows (gol_rule_stream_ragged / gol_gen_stream_ragged) in place
// of the per-generation byte step, whatever the board's size (block rows under a rule do not exist).  The geometry
// takes rows of at least 64 cells.  By default (option "rule_ragged" 1) on calls of at least kRuleRaggedMinGens
// generations -- the pack launch in front of the pass costs a few byte steps -- and on boards above a size floor: the
// byte step's time follows the cells, the streaming passes are latency-bound and flat up to a few million cells
// (profiles/ragged_rules/ragged_rules_bench.json, us/generation at 64 per call, ragged / byte step):
//   life-like (B36/S23)      1001^2 torus 6.0 / 6.2, bounded 5.4 / 7.5; 10001^2 10.5 / 334 and 10.5 / 490
//   Generations (B2/S345/4)  1001^2 torus 7.5 / 6.6, bounded 5.6 / 7.8; 10001^2 14.8 / 367 and 13.7 / 705
// Life-like rules keep the floor of the single-wave pass's 128 x 256 cells (every measured cell of >= 4 generations is
// below the byte step with the state resident; with a pack in the call the 1001^2 torus is 16 % above it at 4
// generations and 2 % at 16).  Generations boards lost on the 1001^2 torus at every call length, so their floor is
// 2^22 cells: between the two measured sizes the byte step interpolates to 17 us there, the pass to under 13 with the
// pack of a 4-generation call.  2 = every board and call the geometry takes (tests, A/B), 0 = never.
constexpr int64_t kRuleRaggedMinGens = 4;
constexpr int64_t kRuleRaggedMinCells = 128 * 256;
constexpr int64_t kGenRaggedMinCells = (int64_t)1 << 22;
bool use_rule_ragged(const gol_board* b, int64_t gens) {
    if (b->packed || b->W % 32 == 0 || b->W < 64 || !b->opt.rule_ragged) return false;
    if (b->opt.rule_ragged == 2) return true;
    return b->W * b->H > (b->nstates > 2 ? kGenRaggedMinCells : kRuleRaggedMinCells) && gens >= kRuleRaggedMinGens;
}

int64_t ring_cells(int64_t W, int64_t H, int boundary) { return gol::ring_pitch(W, boundary == GOL_TORUS) * 32 * H; }

int ring_ilv(const gol_board* b) { return ring_cells(b->W, b->H, b->boundary) < kSmallBoardCells ? 1 : 2; }

void board_layout(gol_board* b, int nparts, int tblock_k, int ilv) {
    const int64_t width = b->W, height = b->H;
    b->packed = (width % 32) == 0;
    b->ilv = b->packed ? (ilv ? ilv : board_ilv(width, height, nparts, b->boundary)) : 0;
    // an explicit depth the level-pipelined layout does not run (12, 24 at ilv 4): the streaming layout by width
    if (b->packed && !ilv && tblock_k && !gol::stream_supported(tblock_k, b->ilv)) b->ilv = pick_ilv(width);
    b->tblock = tblock_k ? tblock_k : board_tblock(b->ilv, width * height, b->boundary);
    if (!b->packed && !tblock_k && ring_by_size(width, height)) {
        // large ragged boards stream as block rows of ring_pitch(W) words: the aligned rules for that many cells
        const int64_t rc = ring_cells(width, height, b->boundary);
        b->tblock = board_tblock(rc < kSmallBoardCells ? 1 : 2, rc, b->boundary);
    }
    b->tblock_set = tblock_k != 0;
    b->pitch = b->packed ? width / 32 : 0;
}

// The pass a gol_step call of `gens` generations takes, first match first (DESIGN.md "Pass order"); the single-wave
// test comes first and costs a few compares: the 100 x 100 board's call latency is a published number.  A packed board
// fails the ragged tests, and a byte board the lanes and cooperative ones, on their first compare.
//
// A board of the rule family (any rule but B3/S23, or the "rule_table" knob; gol_set_rule refuses multi-part boards)
// has four passes: the single-wave kernel with the rule table where it applies, the rule-generic streaming pass
// (gol_rule_step.hip) on every other packed board whatever its layout, the same pass on the scratch rows of the ragged
// byte boards use_rule_ragged takes, and the per-generation byte step under the rule on the byte boards left.  The
// lanes, cooperative, LDS-resident, pipelined and the other ragged passes are B3/S23 only.
//
// A Generations board (nstates > 2, gol_set_generations_rule; single boards only) has three passes whatever its rule:
// the multi-plane streaming pass (gol_gen_stream.hip) on every packed board, the same pass on the scratch rows and decay
// planes of the ragged byte boards use_rule_ragged takes, and the per-generation byte step on the (alive byte, d byte)
// pair on the byte boards left.  The single-wave pass is not taken there.
PassChoice choose_pass(const gol_board* b, int64_t gens) {
    if (b->multi) return {Pass::Multi, 0};
    if (b->nstates > 2) return {b->packed ? kPassGenStream : (use_rule_ragged(b, gens) ? kPassGenRagged : Pass::Bytes), 0};
    if (use_wave_resident(b)) return {Pass::Wave, 0};
    if (b->rule_family())
        return {b->packed ? Pass::RuleStream : (use_rule_ragged(b, gens) ? kPassRuleRagged : Pass::Bytes), 0};
    if (use_lanes(b, gens)) return {Pass::Lanes, 0};
    if (use_coop(b)) return {Pass::Coop, 0};
    int64_t rag_pitch = 0;
    if (gens >= kCoopRaggedMinGens && use_coop_ragged(b, &rag_pitch)) return {Pass::CoopRagged, rag_pitch};
    if (gens >= kStreamRaggedMinGens && use_stream_ragged(b))
        return {use_ring(b) ? Pass::Ring : Pass::StreamRagged, 0};
    if (use_resident(b)) return {Pass::Resident, 0};
    return {b->packed ? Pass::Stream : Pass::Bytes, 0};
}

}  // namespace gol

extern "C" {

int gol_default_ilv(int64_t width) {
    if (width < 32 || width % 32) return 0;
    return gol::pick_ilv(width);
}

int gol_default_tblock(int ilv) {
    if (ilv != 1 && ilv != 2 && ilv != 4) return 0;
    return gol::default_tblock(ilv);
}

int gol_default_layout(int64_t width, int64_t rows, int boundary, int* ilv, int* tblock_k) {
    if (!ilv || !tblock_k) return gol::fail(GOL_ERR_INVALID, "null argument");
    if (width < 32 || width % 32 || rows < 1 || (boundary != GOL_TORUS && boundary != GOL_BOUNDED))
        return gol::fail(GOL_ERR_INVALID, "width must be a positive multiple of 32, rows >= 1, boundary torus or bounded");
    if (gol::pipe_shape(width, rows, boundary)) {
        *ilv = 4;
        *tblock_k = gol::kPipeK;
    } else {
        *ilv = gol::pick_ilv(width);
        *tblock_k = gol::default_tblock(*ilv);
    }
    return GOL_OK;
}

int gol_supported_k(int k, int ilv) { return gol::stream_supported(k, ilv) ? 1 : 0; }

}  // extern "C"
