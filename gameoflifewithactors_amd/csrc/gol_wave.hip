// gol_wave.hip -- single-wave, register-resident pass for the reference-size boards (gfx950).
//
// The reference's own board is 100 x 100 (GameOfLifeLogic.fs:5, GameofLife.fs:18): 10^4 cells, a width that is
// not a multiple of 32.  On such a board every other path is latency-bound: the byte step is one launch per
// generation, the LDS-resident pass (gol_resident.hip) pays a workgroup barrier and LDS round trips per
// generation.  Here ONE wavefront holds the whole board in VGPRs, bit-packed with a masked last word:
//
//   lane L holds rows L*RPL .. L*RPL + RPL-1 (RPL = rows per lane, ceil(H / RPL) <= 64 lanes; gol_wave_body.h has the
//   last lane of a board whose rows do not divide), each as NW = ceil(W / 32) words, bit b of word j = cell 32 j + b,
//   bits >= W zero.
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
#include "gol_wave_dispatch.h"
#include "gol_wave_shape.h"

namespace gol {
namespace {

// PackedRule is empty or one uint32_t, as in gol_batch.hip.  Empty: B3/S23 by life_next, the kernel and its arguments
// as they were before rules existed.  One word: any life-like rule by its packed masks (gol_wave_body.h wave_rule).
// launch_wave_resident picks the family.  PARTIAL: the rows do not divide into lanes and the last lane is partly
// filled (gol_wave_body.h; rule family only, RPL 2..4): the row guards below, and wave_generation's PARTIAL.
template <int NW, int RPL, bool BOUNDED, bool BYTES, bool PARTIAL, class... PackedRule>
__global__ __launch_bounds__(64) void gol_wave_resident(const void* __restrict__ src, void* __restrict__ dst, int W,
                                                        int H, int64_t pitch, int gens, PackedRule... packed_rule) {
    using Rule = decltype(wave_rule(packed_rule...));
    const Rule rule = wave_rule(packed_rule...);
    const int lane = threadIdx.x;
    const int nl = PARTIAL ? (H + RPL - 1) / RPL : H / RPL;    // active lanes
    const int last_rows = PARTIAL ? H - (nl - 1) * RPL : RPL;  // rows of the last one
    // (`PARTIAL &&`: a comparison computed here and left unused still changes the 64 BOUNDED kernels without PARTIAL)
    const bool active = lane < nl, last = PARTIAL && lane == nl - 1;
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
                        if constexpr (PARTIAL) {  // the row clamped into the board too, and a row past it read as zero
                            const int y = L * RPL + i;
                            const uint8_t t = cells[(int64_t)(y < H ? y : H - 1) * W + (x < W ? x : W - 1)];
                            v[b][i][c] = (x < W && y < H) ? t : (uint8_t)0;
                        } else {
                            const uint8_t t = cells[(int64_t)(L * RPL + i) * W + (x < W ? x : W - 1)];
                            v[b][i][c] = x < W ? t : (uint8_t)0;
                        }
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
            if (!PARTIAL || lane * RPL + i < H) {
#pragma unroll
                for (int j = 0; j < NW; j++)
                    w[i][j] = static_cast<const uint32_t*>(src)[(int64_t)(lane * RPL + i) * pitch + j];
            }
    }
    // lanes the rows above the first row / below the last row come from, and the generation itself: gol_wave_body.h
    const WaveGeom geom = wave_geom<BOUNDED>(W, nl, lane);
    for (int g = 0; g < gens; g++) wave_generation<NW, RPL, BOUNDED, Rule, PARTIAL>(w, geom, rule, last, last_rows);

    // ---- store: byte boards row by row, each lane writing one cell of a 64-cell run (the owner lane's two
    // words read as scalars), packed boards one word store per owned word
    if (BYTES) {
        uint8_t* cells = static_cast<uint8_t*>(dst);
        for (int L = 0; L < nl; L++) {
#pragma unroll
            for (int i = 0; i < RPL; i++) {
                if (PARTIAL && L * RPL + i >= H) continue;  // (uniform)
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
        if (!PARTIAL || lane * RPL + i < H) {
#pragma unroll
            for (int j = 0; j < NW; j++)
                static_cast<uint32_t*>(dst)[(int64_t)(lane * RPL + i) * pitch + j] = w[i][j];
        }
}

}  // namespace

// rule: the packed masks (gol_rule.h rule_pack); B3/S23 runs the life_next instantiations, any other rule -- or B3/S23
// with force_table (board option "rule_table") -- the rule-table family, which also takes rows that do not divide into
// lanes (wave_rule_rpl: H % rpl != 0 only there, and only with 2..4 rows per lane).
hipError_t launch_wave_resident(const void* src, void* dst, int64_t W, int64_t H, int64_t pitch, int64_t gens,
                                bool bounded, bool bytes, uint32_t rule, bool force_table, hipStream_t s) {
    const RuleFamily family = rule_family(rule, force_table);
    const int rpl = family == RuleFamily::Table ? wave_rule_rpl(W, H) : wave_resident_rpl(W, H);
    if (!rpl || gens < 1 || gens > INT32_MAX || !rule_packed_ok(rule) || (!bytes && (W % 32 || pitch < W / 32)))
        return hipErrorInvalidValue;
    const int w = (int)W, h = (int)H, n = (int)gens;
    const auto launch = [&](auto NW, auto RPL, auto B, auto Y, auto PARTIAL) {
        if constexpr (!PARTIAL) {
            if (family == RuleFamily::Life) {
                hipLaunchKernelGGL((gol_wave_resident<NW, RPL, B, Y, false>), dim3(1), dim3(64), 0, s, src, dst, w, h,
                                   pitch, n);
                return hipGetLastError();
            }
        }
        if constexpr (!PARTIAL || RPL > 1) {
            if (family == RuleFamily::Table) {
                hipLaunchKernelGGL((gol_wave_resident<NW, RPL, B, Y, PARTIAL, uint32_t>), dim3(1), dim3(64), 0, s, src,
                                   dst, w, h, pitch, n, rule);
                return hipGetLastError();
            }
        }
        return hipErrorInvalidValue;  // no such kernel: a partly filled last lane under B3/S23, or of one row
    };
    return wave_dispatch(launch, (int)((W + 31) / 32), rpl, bounded, bytes, H % rpl != 0);
}

}  // namespace gol
