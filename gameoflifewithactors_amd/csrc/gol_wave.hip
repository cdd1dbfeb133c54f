// gol_wave.hip -- single-wave, register-resident pass for the reference-size boards (gfx950).
//
// The reference's own board is 100 x 100 (GameOfLifeLogic.fs:5, GameofLife.fs:18): 10^4 cells, a width that is
// not a multiple of 32.  On such a board every other path is latency-bound: the byte step is one launch per
// generation, the LDS-resident pass (gol_resident.hip) pays a workgroup barrier and LDS round trips per
// generation.  Here ONE wavefront holds the whole board in VGPRs, bit-packed with a masked last word:
//
//   lane L holds rows L*RPL .. L*RPL + RPL-1 (RPL = rows per lane, H % RPL == 0, H / RPL <= 64 lanes),
//   each as NW = ceil(W / 32) words, bit b of word j = cell 32 j + b, bits >= W zero.
//
// A generation is the synchronous B3/S23 step (GameOfLifeLogic.fs:59-63 under the Reset->State barrier)
// with no barrier and no memory traffic at all: horizontal neighbours by funnel shifts inside the lane, with
// the x-wrap fix-up at the ragged row end (torus, GameOfLifeDriver.fs:21-25; dead outside when bounded,
// Script.fsx:6-13); the row sums of the rows above a lane's first row and below its last row come from the
// neighbouring lanes by ds_bpermute (wrapping from the last active lane to lane 0 on a torus); the rule is
// the streaming kernel's LUT tree (gol_bitlogic.h).  The board is read once and written once per call, from
// and to the board's own storage: bytes (ragged widths, one byte per cell) or packed ilv-1 words.
#include "gol_internal.h"
#include "gol_bitlogic.h"
#include "gol_rule.h"
#include "gol_wave_body.h"

namespace gol {
namespace {

// PackedRule is empty or one uint32_t, as in gol_batch.hip.  Empty: B3/S23 by life_next, the kernel and its arguments
// as they were before rules existed.  One word: any life-like rule by its packed masks (gol_wave_body.h wave_rule).
// launch_wave_resident picks the family.
template <int NW, int RPL, bool BOUNDED, bool BYTES, class... PackedRule>
__global__ __launch_bounds__(64) void gol_wave_resident(const void* __restrict__ src, void* __restrict__ dst, int W,
                                                        int H, int64_t pitch, int gens, PackedRule... packed_rule) {
    const auto rule = wave_rule(packed_rule...);
    const int lane = threadIdx.x;
    const int nl = H / RPL;  // active lanes
    const bool active = lane < nl;
    uint32_t w[RPL][NW];

    // ---- load the board: byte boards row by row, 64 cells per wave-wide coalesced load, packed by ballot (the
    // 64-bit lane mask is the next two words of the row) into the lane that owns the row; packed boards one word
    // load per owned word
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) w[i][j] = 0;
    if (BYTES) {
        // kBatch owner lanes' rows per round: all their loads are issued before the first ballot, so a round
        // waits for memory once (one load, one wait, one ballot per 64 cells cost a memory round trip each:
        // ~30 us of a 100-generation call on the reference's 100^2 board)
        constexpr int kBatch = 8;
        constexpr int kChunks = (NW + 1) / 2;
        const uint8_t* cells = static_cast<const uint8_t*>(src);
        for (int L0 = 0; L0 < nl; L0 += kBatch) {
            uint8_t v[kBatch][RPL][kChunks];
#pragma unroll
            for (int b = 0; b < kBatch; b++)
#pragma unroll
                for (int i = 0; i < RPL; i++)
#pragma unroll
                    for (int c = 0; c < kChunks; c++) {
                        // unconditional loads (address clamped into the board, value masked): a branch per load
                        // would make the compiler wait for each
                        // (owner lanes past the last active lane load a clamped row and keep garbage: no active
                        // lane reads them, and they are never stored)
                        const int x = 64 * c + lane;
                        const int L = L0 + b < nl ? L0 + b : nl - 1;
                        const uint8_t t = cells[(int64_t)(L * RPL + i) * W + (x < W ? x : W - 1)];
                        v[b][i][c] = x < W ? t : (uint8_t)0;
                    }
#pragma unroll
            for (int b = 0; b < kBatch; b++)
#pragma unroll
                for (int i = 0; i < RPL; i++)
#pragma unroll
                    for (int c = 0; c < kChunks; c++) {
                        const uint64_t m = __ballot(v[b][i][c] != 0);
                        if (lane == L0 + b) {
                            w[i][2 * c] = (uint32_t)m;
                            if (2 * c + 1 < NW) w[i][2 * c + 1] = (uint32_t)(m >> 32);
                        }
                    }
        }
    } else if (active) {
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++)
                w[i][j] = static_cast<const uint32_t*>(src)[(int64_t)(lane * RPL + i) * pitch + j];
    }
    // lanes the rows above the first row / below the last row come from, and the generation itself: gol_wave_body.h
    const WaveGeom geom = wave_geom<BOUNDED>(W, nl, lane);
    for (int g = 0; g < gens; g++) wave_generation<NW, RPL, BOUNDED>(w, geom, rule);

    // ---- store: byte boards row by row, each lane writing one cell of a 64-cell run (the owner lane's two
    // words read as scalars), packed boards one word store per owned word
    if (BYTES) {
        uint8_t* cells = static_cast<uint8_t*>(dst);
        for (int L = 0; L < nl; L++) {
#pragma unroll
            for (int i = 0; i < RPL; i++) {
                uint8_t* row = cells + (int64_t)(L * RPL + i) * W;
#pragma unroll
                for (int c = 0; c < (NW + 1) / 2; c++) {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w[i][2 * c], L);
                    const uint32_t hi =
                        2 * c + 1 < NW ? (uint32_t)__builtin_amdgcn_readlane((int)w[i][2 * c + 1], L) : 0u;
                    const int x = 64 * c + lane;
                    const uint32_t word = lane < 32 ? lo : hi;
                    if (x < W) row[x] = (uint8_t)((word >> (lane & 31)) & 1u);
                }
            }
        }
        return;
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) static_cast<uint32_t*>(dst)[(int64_t)(lane * RPL + i) * pitch + j] = w[i][j];
}

template <int NW, int RPL>
hipError_t launch_nr(const void* src, void* dst, int W, int H, int64_t pitch, int gens, bool bounded, bool bytes,
                     bool table, uint32_t rule, hipStream_t s) {
#define GOL_WAVE_LAUNCH(B, Y)                                                                                        \
    if (table)                                                                                                       \
        hipLaunchKernelGGL((gol_wave_resident<NW, RPL, B, Y, uint32_t>), dim3(1), dim3(64), 0, s, src, dst, W, H,    \
                           pitch, gens, rule);                                                                       \
    else                                                                                                             \
        hipLaunchKernelGGL((gol_wave_resident<NW, RPL, B, Y>), dim3(1), dim3(64), 0, s, src, dst, W, H, pitch, gens)
    if (bounded) {
        if (bytes) {
            GOL_WAVE_LAUNCH(true, true);
        } else {
            GOL_WAVE_LAUNCH(true, false);
        }
    } else {
        if (bytes) {
            GOL_WAVE_LAUNCH(false, true);
        } else {
            GOL_WAVE_LAUNCH(false, false);
        }
    }
#undef GOL_WAVE_LAUNCH
    return hipGetLastError();
}

template <int NW>
hipError_t launch_n(const void* src, void* dst, int W, int H, int64_t pitch, int gens, bool bounded, bool bytes, int rpl,
                    bool table, uint32_t rule, hipStream_t s) {
    switch (rpl) {
        case 1: return launch_nr<NW, 1>(src, dst, W, H, pitch, gens, bounded, bytes, table, rule, s);
        case 2: return launch_nr<NW, 2>(src, dst, W, H, pitch, gens, bounded, bytes, table, rule, s);
        case 3: return launch_nr<NW, 3>(src, dst, W, H, pitch, gens, bounded, bytes, table, rule, s);
        case 4: return launch_nr<NW, 4>(src, dst, W, H, pitch, gens, bounded, bytes, table, rule, s);
    }
    return hipErrorInvalidValue;
}

// ---- boards whose rows do not divide into lanes (rule family only; B3/S23 boards never come here: their pass choice
// and their kernels are wave_resident_rpl's, as they were).  nl = ceil(H / RPL) <= 64 lanes, lane L holds rows L RPL ..
// L RPL + RPL - 1 as above, and the last lane only v = H - (nl - 1) RPL of them: its slots v .. RPL - 1 are no rows of
// the board.  They are never loaded (zero), never stored and never read: row H - 1 (slot v - 1 of the last lane) takes
// the sums below it from lane 0's first row (zero on a bounded board) instead of from slot v, and lane 0 takes the
// sums above its first row from slot v - 1 of the last lane instead of from slot RPL - 1.  Everything else is
// wave_generation with the rule table (gol_wave_body.h), whose B0 invariants hold here the same way.
template <int NW, int RPL, bool BOUNDED>
__device__ __forceinline__ void wave_generation_partial(uint32_t (&w)[RPL][NW], const WaveGeom& g, bool last, int v,
                                                        uint32_t rule) {
    uint32_t s[RPL][NW], c[RPL][NW];
#pragma unroll
    for (int i = 0; i < RPL; i++) ragged_row_sum<NW, BOUNDED>(w[i], g.lb, g.lbbit, s[i], c[i]);
    uint32_t ls[NW], lc[NW];  // the sums of the lane's last row of the board
#pragma unroll
    for (int j = 0; j < NW; j++) ls[j] = s[RPL - 1][j], lc[j] = c[RPL - 1][j];
#pragma unroll
    for (int i = 0; i + 1 < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) {
            ls[j] = (last && v - 1 == i) ? s[i][j] : ls[j];
            lc[j] = (last && v - 1 == i) ? c[i][j] : lc[j];
        }
    uint32_t us[NW], uc[NW], ds[NW], dc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
        us[j] = bperm(g.up_addr, ls[j]) & g.up_mask;
        uc[j] = bperm(g.up_addr, lc[j]) & g.up_mask;
        ds[j] = bperm(g.dn_addr, s[0][j]) & g.dn_mask;
        dc[j] = bperm(g.dn_addr, c[0][j]) & g.dn_mask;
    }
#pragma unroll
    for (int i = 0; i < RPL; i++) {
        uint32_t sN[NW], cN[NW], o[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) {
            const bool below_is_lane0 = i == RPL - 1 || (last && v - 1 == i);
            sN[j] = below_is_lane0 ? ds[j] : s[i + 1 < RPL ? i + 1 : i][j];
            cN[j] = below_is_lane0 ? dc[j] : c[i + 1 < RPL ? i + 1 : i][j];
        }
        rule_next_row<NW>(i == 0 ? us : s[i - 1], i == 0 ? uc : c[i - 1], s[i], c[i], sN, cN, w[i], rule, o);
#pragma unroll
        for (int j = 0; j < NW; j++) w[i][j] = j == NW - 1 ? o[j] & g.lastmask : o[j];
    }
}

template <int NW, int RPL, bool BOUNDED, bool BYTES>
__global__ __launch_bounds__(64) void gol_wave_rule_partial(const void* __restrict__ src, void* __restrict__ dst, int W,
                                                            int H, int64_t pitch, int gens, uint32_t rule) {
    const int lane = threadIdx.x;
    const int nl = (H + RPL - 1) / RPL;   // active lanes
    const int v = H - (nl - 1) * RPL;     // rows of the last one
    const bool active = lane < nl, last = lane == nl - 1;
    uint32_t w[RPL][NW];
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) w[i][j] = 0;
    if (BYTES) {  // as gol_wave_resident, the row clamped into the board and a row past it read as zero
        constexpr int kBatch = 8;
        constexpr int kChunks = (NW + 1) / 2;
        const uint8_t* cells = static_cast<const uint8_t*>(src);
        for (int L0 = 0; L0 < nl; L0 += kBatch) {
            uint8_t t[kBatch][RPL][kChunks];
#pragma unroll
            for (int b = 0; b < kBatch; b++)
#pragma unroll
                for (int i = 0; i < RPL; i++)
#pragma unroll
                    for (int c = 0; c < kChunks; c++) {
                        const int x = 64 * c + lane;
                        const int L = L0 + b < nl ? L0 + b : nl - 1;
                        const int y = L * RPL + i;
                        const uint8_t q = cells[(int64_t)(y < H ? y : H - 1) * W + (x < W ? x : W - 1)];
                        t[b][i][c] = (x < W && y < H) ? q : (uint8_t)0;
                    }
#pragma unroll
            for (int b = 0; b < kBatch; b++)
#pragma unroll
                for (int i = 0; i < RPL; i++)
#pragma unroll
                    for (int c = 0; c < kChunks; c++) {
                        const uint64_t m = __ballot(t[b][i][c] != 0);
                        if (lane == L0 + b) {
                            w[i][2 * c] = (uint32_t)m;
                            if (2 * c + 1 < NW) w[i][2 * c + 1] = (uint32_t)(m >> 32);
                        }
                    }
        }
    } else if (active) {
#pragma unroll
        for (int i = 0; i < RPL; i++)
            if (lane * RPL + i < H) {
#pragma unroll
                for (int j = 0; j < NW; j++)
                    w[i][j] = static_cast<const uint32_t*>(src)[(int64_t)(lane * RPL + i) * pitch + j];
            }
    }
    const WaveGeom geom = wave_geom<BOUNDED>(W, nl, lane);
    for (int g = 0; g < gens; g++) wave_generation_partial<NW, RPL, BOUNDED>(w, geom, last, v, rule);

    if (BYTES) {
        uint8_t* cells = static_cast<uint8_t*>(dst);
        for (int L = 0; L < nl; L++) {
#pragma unroll
            for (int i = 0; i < RPL; i++) {
                const int y = L * RPL + i;  // (uniform)
                if (y >= H) continue;
                uint8_t* row = cells + (int64_t)y * W;
#pragma unroll
                for (int c = 0; c < (NW + 1) / 2; c++) {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w[i][2 * c], L);
                    const uint32_t hi =
                        2 * c + 1 < NW ? (uint32_t)__builtin_amdgcn_readlane((int)w[i][2 * c + 1], L) : 0u;
                    const int x = 64 * c + lane;
                    const uint32_t word = lane < 32 ? lo : hi;
                    if (x < W) row[x] = (uint8_t)((word >> (lane & 31)) & 1u);
                }
            }
        }
        return;
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < RPL; i++)
        if (lane * RPL + i < H) {
#pragma unroll
            for (int j = 0; j < NW; j++)
                static_cast<uint32_t*>(dst)[(int64_t)(lane * RPL + i) * pitch + j] = w[i][j];
        }
}

template <int NW, int RPL>
hipError_t launch_partial_nr(const void* src, void* dst, int W, int H, int64_t pitch, int gens, bool bounded, bool bytes,
                             uint32_t rule, hipStream_t s) {
#define GOL_WAVE_LAUNCH(B, Y) \
    hipLaunchKernelGGL((gol_wave_rule_partial<NW, RPL, B, Y>), dim3(1), dim3(64), 0, s, src, dst, W, H, pitch, gens, rule)
    if (bounded) {
        if (bytes) {
            GOL_WAVE_LAUNCH(true, true);
        } else {
            GOL_WAVE_LAUNCH(true, false);
        }
    } else {
        if (bytes) {
            GOL_WAVE_LAUNCH(false, true);
        } else {
            GOL_WAVE_LAUNCH(false, false);
        }
    }
#undef GOL_WAVE_LAUNCH
    return hipGetLastError();
}

template <int NW>
hipError_t launch_partial_n(const void* src, void* dst, int W, int H, int64_t pitch, int gens, bool bounded, bool bytes,
                            int rpl, uint32_t rule, hipStream_t s) {
    switch (rpl) {
        case 2: return launch_partial_nr<NW, 2>(src, dst, W, H, pitch, gens, bounded, bytes, rule, s);
        case 3: return launch_partial_nr<NW, 3>(src, dst, W, H, pitch, gens, bounded, bytes, rule, s);
        case 4: return launch_partial_nr<NW, 4>(src, dst, W, H, pitch, gens, bounded, bytes, rule, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// Rows per lane for an H-row board: the fewest (1..4) that divide H with at most 64 lanes, or 0.
int wave_resident_rpl(int64_t W, int64_t H) {
    if (W < 3 || W > 128 || H < 3) return 0;
    for (int r = 1; r <= 4; r++)
        if (H % r == 0 && H / r <= 64) return r;
    return 0;
}

// Rows per lane under the rule family: wave_resident_rpl where it takes the board, else the fewest (2..4) that hold H
// rows in at most 64 lanes with the last lane partly filled (gol_wave_rule_partial), or 0.  Every board up to 128 x 256.
int wave_rule_rpl(int64_t W, int64_t H) {
    if (const int r = wave_resident_rpl(W, H)) return r;
    if (W < 3 || W > 128 || H < 3) return 0;
    for (int r = 2; r <= 4; r++)
        if ((H + r - 1) / r <= 64) return r;
    return 0;
}

// rule: the packed masks (gol_rule.h rule_pack); B3/S23 runs the life_next instantiations, any other rule -- or B3/S23
// with force_table (board option "rule_table") -- the rule-table family.
hipError_t launch_wave_resident(const void* src, void* dst, int64_t W, int64_t H, int64_t pitch, int64_t gens,
                                bool bounded, bool bytes, uint32_t rule, bool force_table, hipStream_t s) {
    const bool table = force_table || rule != kRuleLifePacked;  // B3/S23 runs the code it always ran
    const int rpl = table ? wave_rule_rpl(W, H) : wave_resident_rpl(W, H);
    if (!rpl || gens < 1 || gens > INT32_MAX || rule >= (1u << 18) || (!bytes && (W % 32 || pitch < W / 32)))
        return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    if (H % rpl) {  // rows that do not divide into lanes: the rule family's own kernel
        switch (nw) {
            case 1: return launch_partial_n<1>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, rule, s);
            case 2: return launch_partial_n<2>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, rule, s);
            case 3: return launch_partial_n<3>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, rule, s);
            case 4: return launch_partial_n<4>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, rule, s);
        }
        return hipErrorInvalidValue;
    }
    switch (nw) {
        case 1: return launch_n<1>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, table, rule, s);
        case 2: return launch_n<2>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, table, rule, s);
        case 3: return launch_n<3>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, table, rule, s);
        case 4: return launch_n<4>(src, dst, (int)W, (int)H, pitch, (int)gens, bounded, bytes, rpl, table, rule, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace gol
