// gol_cycles.hip -- the ensemble cycle census (gol_ensemble_cycles): for every board of a batch, after
// how many generations it enters a cycle and of what period, one wavefront per board, in one launch (gfx950).
//
// A wave loads its board into registers as the batch step does (gol_batch.hip: same layout, same geometry, lane L holds
// rows L*RPL ..), and runs the search of gol_cycle_search.h on it: the generation is wave_generation (gol_wave_body.h),
// two boards are compared in registers, and nothing is stored but the board's four result words.  The boards are const.
//
// Every lane of the wave runs every generation (the row exchange reads its neighbours' registers), so every branch of
// the search must be wave-uniform: `equal` reduces the lanes' differences with one ballot, whose result is a scalar,
// and the search's counters depend on nothing else.
#include "gol_batch_host.h"
#include "gol_cycle_search.h"
#include "gol_internal.h"
#include "gol_rule.h"
#include "gol_wave_body.h"
#include "gol_wave_dispatch.h"

namespace gol {
namespace {

template <class Rule>
struct CycleWave {
    WaveGeom geom;
    Rule rule;  // gol_wave_body.h RuleLife / RuleTable
    uint64_t lanes;  // the lanes that hold rows of the board: what the others hold never counts as a difference
};

// One board in the wave's registers, as the search's state type.
template <int NW, int RPL, bool BOUNDED, class Rule>
struct WaveBoard {
    uint32_t w[RPL][NW];
    const CycleWave<Rule>* wave;

    __device__ __forceinline__ void step() { wave_generation<NW, RPL, BOUNDED>(w, wave->geom, wave->rule); }
    // the same value in every lane: each lane ORs the XOR of its words (one v_bitop3 per word), one ballot
    __device__ __forceinline__ bool equal(const WaveBoard& o) const {
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) d = lut3<0xBE>(d, w[i][j], o.w[i][j]);  // d | (a ^ b)
        return (__ballot(d != 0) & wave->lanes) == 0;
    }
};

// Board blockIdx.x: out[4 board ..] = transient, period, population of B_transient, generation steps run.
// PackedRule is empty (B3/S23 by life_next: the kernel as it was before rules existed), one uint32_t (any life-like
// rule by its packed masks) or one const uint32_t* (`count` packed rules, the wave's own read once as a scalar after
// the test on `board`), as in gol_batch.hip: launch_batch_cycles picks.
template <int NW, int RPL, bool BOUNDED, class... PackedRule>
__global__ __launch_bounds__(64) void gol_batch_cycles(const uint32_t* __restrict__ words, int64_t count, int W, int H,
                                                       int max_generations, int32_t* __restrict__ out,
                                                       PackedRule... packed_rule) {
    const int lane = threadIdx.x;
    const int64_t board = blockIdx.x;
    if (board >= count) return;
    using Rule = decltype(board_rule(board, packed_rule...));
    const int nl = H / RPL;  // active lanes
    const bool active = lane < nl;
    const uint32_t* rows = words + (board * H + lane * RPL) * NW;  // this lane's RPL * NW words
    CycleWave<Rule> cw;
    cw.geom = wave_geom<BOUNDED>(W, nl, lane);
    cw.rule = board_rule(board, packed_rule...);
    cw.lanes = __ballot(active);
    using Board = WaveBoard<NW, RPL, BOUNDED, Rule>;
    const auto load = [&]() {
        Board b;
        b.wave = &cw;
        wave_load_rows(b.w, rows, active);
        return b;
    };
    uint32_t pop = 0;
    const CycleResult r = cycle_search<Board>(load, max_generations,
                                              [&](const Board& a) { pop = wave_population(a.w, active); });
    if (lane == 0) {
        int32_t* o = out + 4 * board;
        o[0] = r.transient;
        o[1] = r.period;
        o[2] = (int32_t)pop;
        o[3] = r.steps;
    }
}

}  // namespace

hipError_t launch_batch_cycles(const uint32_t* words, int64_t count, int64_t W, int64_t H, bool bounded,
                               int64_t max_generations, int32_t* out, uint32_t rule, bool force_table,
                               const uint32_t* rules, hipStream_t s) {
    const int rpl = wave_resident_rpl(W, H);
    if (!rpl || !rule_packed_ok(rule) || !words || !out || count < 1 || count > kBatchCountMax ||
        max_generations < 1 || max_generations > kCycleGenerationsMax)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)count), block(64);  // count <= 2^22
    const int w = (int)W, h = (int)H, G = (int)max_generations;
    const auto launch = [&](auto NW, auto RPL, auto B) {
        switch (rule_family(rule, force_table, rules)) {
            case RuleFamily::Life:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B>), grid, block, 0, s, words, count, w, h, G, out);
                break;
            case RuleFamily::Table:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B, uint32_t>), grid, block, 0, s, words, count, w, h, G,
                                   out, rule);
                break;
            case RuleFamily::PerBoard:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B, const uint32_t*>), grid, block, 0, s, words, count, w,
                                   h, G, out, rules);
                break;
        }
        return hipGetLastError();
    };
    return wave_dispatch(launch, (int)((W + 31) / 32), rpl, bounded);
}

}  // namespace gol
