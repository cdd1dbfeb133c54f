// gol_wave_body.h -- one generation of a board held in one wavefront's registers: the arithmetic the single-wave
// pass (gol_wave.hip), the batch pass (gol_batch.hip, one wave per board) and the cycle census (gol_cycles.hip) share,
// and the wave-wide sum the batch's population trace and the census use.
//
//   lane L holds rows L*RPL .. L*RPL + RPL-1 (RPL = rows per lane, nl = ceil(H / RPL) <= 64 active lanes),
//   each as NW = ceil(W / 32) words, bit b of word j = cell 32 j + b, bits >= W zero.
//
// Lanes at or beyond nl run the same instructions on whatever they hold: no active lane reads them (a lane's upper
// neighbour is lane - 1, or nl - 1 for lane 0; its lower one lane + 1, or 0 for lane nl - 1), and they are never
// stored.
//
// H % RPL == 0 everywhere but under PARTIAL (gol_wave.hip, rule family only: gol_wave_shape.h wave_rule_rpl; B3/S23
// boards never come there, their pass choice and their kernels are wave_resident_rpl's).  PARTIAL: the rows do not
// divide into lanes, and the last lane holds only v = H - (nl - 1) RPL of them (`last_rows` below): its slots v ..
// RPL - 1 are no rows of the board.  They are never loaded (zero), never stored and never read: row H - 1 (slot v - 1
// of the last lane) takes the sums below it from lane 0's first row (zero on a bounded board) instead of from slot v,
// and lane 0 takes the sums above its first row from slot v - 1 of the last lane instead of from slot RPL - 1.
// Everything else is the rule-table generation as it is where the rows divide, and its B0 invariants hold here the
// same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gol_bitlogic.h"

namespace gol {

__device__ __forceinline__ uint32_t bperm(int byte_addr, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
}

// Horizontal 3-sums of one ragged row (NW words, last word holding bits [0, lb]).
template <int NW, bool BOUNDED>
__device__ __forceinline__ void ragged_row_sum(const uint32_t (&w)[NW], int lb, uint32_t lbbit, uint32_t (&s)[NW],
                                               uint32_t (&c)[NW]) {
    // west neighbour of cell 0 is cell W-1 (bit lb of the last word), moved to bit 31 of a carry word
    const uint32_t wcarry = BOUNDED ? 0u : w[NW - 1] << (31 - lb);
    uint32_t west[NW], east[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) west[j] = align_right(w[j], j == 0 ? wcarry : w[j - 1], 31);
#pragma unroll
    for (int j = 0; j + 1 < NW; j++) east[j] = align_right(w[j + 1], w[j], 1);
    // east neighbour of cell W-1 is cell 0: bit 0 of word 0 into bit lb of the last word
    if (BOUNDED)
        east[NW - 1] = w[NW - 1] >> 1;
    else
        east[NW - 1] = lut3<0xEA>(w[NW - 1] >> 1, w[0] << lb, lbbit);  // a | (b & c)
#pragma unroll
    for (int j = 0; j < NW; j++) {
        s[j] = lut3<0x96>(west[j], w[j], east[j]);
        c[j] = lut3<0xE8>(west[j], w[j], east[j]);
    }
}

// What a lane needs beside its rows: the row end, and the lanes its outer rows' neighbours come from.
struct WaveGeom {
    int lb;             // bit of the row's last cell in the last word, (W - 1) & 31
    uint32_t lbbit;     // 1 << lb
    uint32_t lastmask;  // the last word's cells
    int up_addr, dn_addr;       // ds_bpermute byte addresses of the lanes above / below
    uint32_t up_mask, dn_mask;  // 0 where that row lies outside a bounded board
};

template <bool BOUNDED>
__device__ __forceinline__ WaveGeom wave_geom(int W, int nl, int lane) {
    WaveGeom g;
    g.lb = (W - 1) & 31;
    g.lbbit = 1u << g.lb;
    g.lastmask = g.lb == 31 ? 0xffffffffu : (g.lbbit << 1) - 1u;
    const int up_lane = lane == 0 ? nl - 1 : lane - 1;
    const int dn_lane = lane + 1 >= nl ? 0 : lane + 1;
    g.up_addr = up_lane * 4;
    g.dn_addr = dn_lane * 4;
    g.up_mask = (BOUNDED && lane == 0) ? 0u : 0xffffffffu;  // dead rows outside a bounded board
    g.dn_mask = (BOUNDED && lane == nl - 1) ? 0u : 0xffffffffu;
    return g;
}

// The rule of a generation, as a policy of wave_generation.  RuleLife is B3/S23 by life_next's LUT tree (the code every
// pass had before rules existed); RuleTable is any life-like rule, its packed masks (gol_rule.h rule_pack: a kernel
// argument, so uniform over the launch, or a batch's per-board table entry, uniform over the wave) evaluated by
// rule_next_row.
struct RuleLife {};
struct RuleTable {
    uint32_t packed;
};
// The policy of a kernel whose trailing arguments are nothing (B3/S23) or the packed rule.
__device__ __forceinline__ RuleLife wave_rule() { return RuleLife(); }
__device__ __forceinline__ RuleTable wave_rule(uint32_t packed) { return RuleTable{packed}; }
// The policy of a batch kernel's wave for its board: the two above whatever the board, or, where the trailing argument
// is a table of one packed rule per board (gol_ensemble_set_rules), that board's entry.  `board` is wave-uniform, so
// the entry is one scalar load, and the readfirstlane says so to the compiler wherever it cannot prove it: the rule
// stays in a scalar register and rule_next_row's tests stay scalar, as under the launch-wide rule.
__device__ __forceinline__ RuleLife board_rule(int64_t) { return RuleLife(); }
__device__ __forceinline__ RuleTable board_rule(int64_t, uint32_t packed) { return RuleTable{packed}; }
__device__ __forceinline__ RuleTable board_rule(int64_t board, const uint32_t* rules) {
    return RuleTable{(uint32_t)__builtin_amdgcn_readfirstlane((int)rules[board])};
}

// One synchronous generation of the wave's board, in place in w.  Whatever the rule gives birth on: a row outside a
// bounded board contributes zero sums (up_mask / dn_mask) and is no cell of the board, the last word is cut to the
// row's cells (lastmask) before it is stored in w, and what lanes at or beyond nl hold is never read by an active lane.
// PARTIAL (above): `last` = this is lane nl - 1, which holds `last_rows` (1 .. RPL - 1) rows of the board.
template <int NW, int RPL, bool BOUNDED, class Rule = RuleLife, bool PARTIAL = false>
__device__ __forceinline__ void wave_generation(uint32_t (&w)[RPL][NW], const WaveGeom& g, Rule rule = Rule(),
                                                bool last = false, int last_rows = RPL) {
    static_assert(!(PARTIAL && std::is_same<Rule, RuleLife>::value), "a partly filled last lane: rule family only");
    uint32_t s[RPL][NW], c[RPL][NW];
#pragma unroll
    for (int i = 0; i < RPL; i++) ragged_row_sum<NW, BOUNDED>(w[i], g.lb, g.lbbit, s[i], c[i]);
    uint32_t ls[NW], lc[NW];  // PARTIAL: the sums of the lane's last row of the board (else s[RPL - 1], read in place)
    if constexpr (PARTIAL) {
#pragma unroll
        for (int j = 0; j < NW; j++) ls[j] = s[RPL - 1][j], lc[j] = c[RPL - 1][j];
#pragma unroll
        for (int i = 0; i + 1 < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) {
                ls[j] = (last && last_rows - 1 == i) ? s[i][j] : ls[j];
                lc[j] = (last && last_rows - 1 == i) ? c[i][j] : lc[j];
            }
    }
    uint32_t us[NW], uc[NW], ds[NW], dc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
        us[j] = bperm(g.up_addr, PARTIAL ? ls[j] : s[RPL - 1][j]) & g.up_mask;
        uc[j] = bperm(g.up_addr, PARTIAL ? lc[j] : c[RPL - 1][j]) & g.up_mask;
        ds[j] = bperm(g.dn_addr, s[0][j]) & g.dn_mask;
        dc[j] = bperm(g.dn_addr, c[0][j]) & g.dn_mask;
    }
    if constexpr (std::is_same<Rule, RuleLife>::value) {
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const uint32_t sP = i == 0 ? us[j] : s[i - 1][j], cP = i == 0 ? uc[j] : c[i - 1][j];
                const uint32_t sN = i == RPL - 1 ? ds[j] : s[i + 1][j], cN = i == RPL - 1 ? dc[j] : c[i + 1][j];
                uint32_t v = life_next(sP, cP, s[i][j], c[i][j], sN, cN, w[i][j]);
                if (j == NW - 1) v &= g.lastmask;
                w[i][j] = v;
            }
    } else {
#pragma unroll
        for (int i = 0; i < RPL; i++) {
            uint32_t v[NW];
            if constexpr (PARTIAL) {  // the row below the board's last row is lane 0's first, whatever its slot
                uint32_t sN[NW], cN[NW];
#pragma unroll
                for (int j = 0; j < NW; j++) {
                    const bool below_is_lane0 = i == RPL - 1 || (last && last_rows - 1 == i);
                    sN[j] = below_is_lane0 ? ds[j] : s[i + 1 < RPL ? i + 1 : i][j];
                    cN[j] = below_is_lane0 ? dc[j] : c[i + 1 < RPL ? i + 1 : i][j];
                }
                rule_next_row<NW>(i == 0 ? us : s[i - 1], i == 0 ? uc : c[i - 1], s[i], c[i], sN, cN, w[i], rule.packed,
                                  v);
            } else {
                rule_next_row<NW>(i == 0 ? us : s[i - 1], i == 0 ? uc : c[i - 1], s[i], c[i],
                                  i == RPL - 1 ? ds : s[i + 1], i == RPL - 1 ? dc : c[i + 1], w[i], rule.packed, v);
            }
#pragma unroll
            for (int j = 0; j < NW; j++) w[i][j] = j == NW - 1 ? v[j] & g.lastmask : v[j];
        }
    }
}

// Sum of v over the wave's 64 lanes, the same value in every lane: four DPP adds leave every lane of a row of 16 with
// the row's sum (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror), then the four rows' sums are
// read as scalars.  Every lane of the wave must be executing.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_read(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += dpp_read<0xB1>(v);
    v += dpp_read<0x4E>(v);
    v += dpp_read<0x141>(v);
    v += dpp_read<0x140>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// A lane's RPL x NW words from `rows` (rows back to back, as in a batch), zero in a lane that holds no rows: its `rows`
// points past its board and is never dereferenced.
template <int NW, int RPL>
__device__ __forceinline__ void wave_load_rows(uint32_t (&w)[RPL][NW], const uint32_t* rows, bool active) {
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) w[i][j] = 0;
    if (active) {
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) w[i][j] = rows[i * NW + j];
    }
}

// The board's population, the same value in every lane.  Lanes past the last active one hold whatever the arithmetic
// left there: they count as 0.  Every lane of the wave must be executing.
template <int NW, int RPL>
__device__ __forceinline__ uint32_t wave_population(const uint32_t (&w)[RPL][NW], bool active) {
    uint32_t pop = 0;
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) pop += __popc(w[i][j]);
    return wave_sum_u32(active ? pop : 0u);
}

}  // namespace gol
