// gol_batch_wave.h -- what a batch's wave does with its board in registers (device only): the board's planes, their load,
// one generation, and the cycle census, for the life-like batch (no decay plane) and the Generations batch (1..3 decay
// planes, gol_generations.h) alike.  gol_batch.hip's step kernels and gol_cycles.hip's census kernels are thin entry
// points over it.
//
// Storage.  The alive plane is the batch's `words`: boards back to back, board i row y = NW = ceil(W / 32) words at
// words[(i * H + y) * NW], bit b of word j = cell 32 j + b, bits at or beyond W zero.  Decay plane k (0 .. P - 1,
// P = gen_planes(nstates); none at 2 states) is a whole further array of the same shape at words + (k + 1) *
// plane_stride, plane_stride = count * H * NW words: a cell's word sits at the same index in every plane.  A dying cell
// in state s holds d = s - 1 as a binary number, bit k in plane k; a dead or alive cell holds 0.
//
// Geometry: gol_wave_body.h's (lane L holds rows L*RPL .., NW words each, wave_dispatch picks NW and RPL).  The alive
// plane advances through wave_generation -- only state-1 cells are neighbours -- and the decay planes by gen_decay, per
// word, with no cross-lane traffic.  nstates is a kernel argument (P scalar masks).
//
// Invariants.  Pad bits: wave_generation cuts the alive plane's last word (lastmask) before gen_decay sees it, and
// gen_decay keeps a bit zero in every plane where the old alive plane and the old decay planes had it zero.  Lanes at
// or beyond nl load zeros, run the same instructions on whatever the row exchange leaves them, are read by no active
// lane (wave_geom's addresses), count for nothing (`active` in the population, `lanes` in the census) and are never
// stored.  Rows outside a bounded board contribute nothing: up_mask / dn_mask in wave_generation, and the decay needs
// no neighbour.
//
// The census.  Every lane of the wave runs every generation (the row exchange reads its neighbours' registers), so
// every branch of the search (gol_cycle_search.h) must be wave-uniform: `equal` reduces the lanes' differences with one
// ballot, whose result is a scalar, and the search's counters depend on nothing else.  Nothing is stored but the
// board's four result words; the boards are const.
#pragma once
#include "gol_cycle_search.h"
#include "gol_generations.h"
#include "gol_wave_body.h"

namespace gol {

// One board in one wave's registers: the alive plane and P decay planes.
template <int NW, int RPL, int P>
struct BoardRegs {
    uint32_t a[RPL][NW];
    uint32_t d[P][RPL][NW];
};
template <int NW, int RPL>
struct BoardRegs<NW, RPL, 0> {
    uint32_t a[RPL][NW];
};

// A Generations kernel's rule: the launch's one packed word, or its board's entry of the table (a null test and one
// scalar load per wave).  The third of gol_wave_body.h's board_rule overloads.
__device__ __forceinline__ RuleTable board_rule(int64_t board, uint32_t packed, const uint32_t* rules) {
    return rules ? board_rule(board, rules) : RuleTable{packed};
}

// `rows`: this lane's RPL * NW words of the alive plane (gol_wave_body.h wave_load_rows).
template <int NW, int RPL, int P>
__device__ __forceinline__ void board_load(BoardRegs<NW, RPL, P>& b, const uint32_t* rows, int64_t plane_stride,
                                           bool active) {
    wave_load_rows(b.a, rows, active);
    if constexpr (P > 0) {
#pragma unroll
        for (int k = 0; k < P; k++) wave_load_rows(b.d[k], rows + (k + 1) * plane_stride, active);
    }
}

// What a wave needs beside its board.
template <class Rule>
struct BoardWave {
    WaveGeom geom;
    Rule rule;       // gol_wave_body.h RuleLife / RuleTable
    GenMasks masks;  // gen_masks(nstates); unused without decay planes
    uint64_t lanes;  // the lanes that hold rows of the board: what the others hold never counts as a difference
};

// One synchronous generation of the wave's board, in place.
template <int NW, int RPL, bool BOUNDED, int P, class Rule>
__device__ __forceinline__ void board_generation(BoardRegs<NW, RPL, P>& b, const BoardWave<Rule>& w) {
    if constexpr (P == 0) {
        wave_generation<NW, RPL, BOUNDED>(b.a, w.geom, w.rule);
    } else {
        uint32_t old[RPL][NW];
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) old[i][j] = b.a[i][j];
        wave_generation<NW, RPL, BOUNDED>(b.a, w.geom, w.rule);  // v, its last word cut to the row's cells
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) {
                uint32_t d[P];
#pragma unroll
                for (int k = 0; k < P; k++) d[k] = b.d[k][i][j];
                b.a[i][j] = gen_decay<P>(old[i][j], b.a[i][j], d, w.masks);
#pragma unroll
                for (int k = 0; k < P; k++) b.d[k][i][j] = d[k];
            }
    }
}

// One board in the wave's registers, as the search's state type.
template <int NW, int RPL, bool BOUNDED, int P, class Rule>
struct CycleBoard {
    BoardRegs<NW, RPL, P> b;
    const BoardWave<Rule>* wave;

    __device__ __forceinline__ void step() { board_generation<NW, RPL, BOUNDED, P>(b, *wave); }
    // the same value in every lane: each lane ORs the XOR of its words (one v_bitop3 per word), one ballot
    __device__ __forceinline__ bool equal(const CycleBoard& o) const {
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) {
                diff = lut3<0xBE>(diff, b.a[i][j], o.b.a[i][j]);  // d | (a ^ b)
                if constexpr (P > 0) {
#pragma unroll
                    for (int k = 0; k < P; k++) diff = lut3<0xBE>(diff, b.d[k][i][j], o.b.d[k][i][j]);
                }
            }
        return (__ballot(diff != 0) & wave->lanes) == 0;
    }
};

// The census of `board` by the wave whose lanes are `lane` 0..63: out[4 board ..] = transient, period, state-1 cells of
// B_transient, generation steps run.  packed_rule: what board_rule takes behind `board` -- nothing (B3/S23 by
// life_next), one packed word, a table of one per board, or a word and a table that may be null.
template <int NW, int RPL, bool BOUNDED, int P, class... PackedRule>
__device__ __forceinline__ void board_census(const uint32_t* words, int64_t plane_stride, int64_t board, int lane, int W,
                                             int H, int max_generations, int32_t* out, int nstates,
                                             PackedRule... packed_rule) {
    using Rule = decltype(board_rule(board, packed_rule...));
    const int nl = H / RPL;  // active lanes
    const bool active = lane < nl;
    const uint32_t* rows = words + (board * H + lane * RPL) * NW;  // this lane's RPL * NW words
    BoardWave<Rule> cw;
    cw.geom = wave_geom<BOUNDED>(W, nl, lane);
    cw.rule = board_rule(board, packed_rule...);
    if constexpr (P > 0) cw.masks = gen_masks(nstates);
    cw.lanes = __ballot(active);
    using Board = CycleBoard<NW, RPL, BOUNDED, P, Rule>;
    const auto load = [&]() {
        Board s;
        s.wave = &cw;
        board_load(s.b, rows, plane_stride, active);
        return s;
    };
    uint32_t pop = 0;
    const CycleResult r = cycle_search<Board>(load, max_generations,
                                              [&](const Board& s) { pop = wave_population(s.b.a, active); });
    if (lane == 0) {
        int32_t* o = out + 4 * board;
        o[0] = r.transient;
        o[1] = r.period;
        o[2] = (int32_t)pop;
        o[3] = r.steps;
    }
}

}  // namespace gol
