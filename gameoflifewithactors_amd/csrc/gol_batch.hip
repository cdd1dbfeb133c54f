// gol_batch.hip -- a batch of small boards, one wavefront per board, any number of boards per launch (gfx950).
//
// The reference's board is 100 x 100, seeded from the clock (GameOfLifeLogic.fs:5, GameOfLifeDriver.fs:9-11): every run
// is another member of one ensemble.  The single-wave pass (gol_wave.hip) steps one such board on one of the chip's
// 1024 SIMDs; here `count` boards of one geometry are stepped by `count` waves in one launch, each wave alone with its
// board: it loads the board into registers, runs every generation of the call there (gol_wave_body.h: the arithmetic
// of the single-wave pass, no barrier, no memory traffic) and stores it back to the same place.
//
// Layout: boards back to back, board i row y = NW = ceil(W / 32) words at words[(i * H + y) * NW], bit b of word j =
// cell 32 j + b, bits at or beyond W zero.  In place: a wave reads its whole board before it writes any of it, and no
// wave touches another board.  Geometry: the single-wave pass's (wave_resident_rpl: W 3..128, 1..4 rows per lane on at
// most 64 lanes).  Under a Generations rule (2..8 states per cell) the board has 1..3 decay planes behind this one:
// gol_batch_wave.h has their layout, the board in registers and its generation, and gol_gen_step below runs them.
//
// Also here, one kernel each for every number of states: the per-board observables (gol_batch_observe), the byte forms
// of the cells (gol_batch_pack / gol_batch_unpack) and the splitmix seeding of the alive plane.
#include "gol_batch_host.h"
#include "gol_batch_wave.h"
#include "gol_hash.h"
#include "gol_internal.h"
#include "gol_rule.h"
#include "gol_wave_dispatch.h"

namespace gol {
namespace {

// Board `blockIdx.x * waves per group + wave` runs `samples` x `every` generations.  TRACE: after each `every`
// generations the board's population goes to trace[t * count + board] (t = 0 .. samples - 1); otherwise samples is 1
// and trace unused.  A wave past the last board leaves before it touches memory.
//
// PackedRule is empty, one uint32_t or one const uint32_t*.  Empty: B3/S23 by life_next, the kernel and its arguments
// as they were before rules existed.  One word: any life-like rule by its packed masks (gol_wave_body.h board_rule).
// A pointer: `count` packed rules, one per board (gol_ensemble_set_rules); the wave reads its own once, as a scalar,
// after the test that sends a wave past the last board away and before it loads its board, so the waves of one
// workgroup may run different rules: each takes its own scalar branches in rule_next_row.  launch_batch_step picks the
// family; nothing else lets a rule change what runs.
template <int NW, int RPL, bool BOUNDED, bool TRACE, class... PackedRule>
__global__ __launch_bounds__(256) void gol_batch_step(uint32_t* __restrict__ words, int64_t count, int W, int H,
                                                      int samples, int64_t every, uint32_t* __restrict__ trace,
                                                      PackedRule... packed_rule) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t board = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (board >= count) return;
    const auto rule = board_rule(board, packed_rule...);
    const int nl = H / RPL;  // active lanes
    const bool active = lane < nl;
    uint32_t* rows = words + (board * H + lane * RPL) * NW;  // this lane's RPL * NW words
    uint32_t w[RPL][NW];
    // (gol_wave_body.h wave_load_rows, inline: through the helper 179 of this file's 196 kernels compile differently;
    // and these very lines behind a function call, for one body with gol_gen_step, 70 of these 192: DESIGN.md 4.9)
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) w[i][j] = 0;
    if (active) {  // (an inactive lane's `rows` points past its board: never dereferenced)
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) w[i][j] = rows[i * NW + j];
    }
    const WaveGeom geom = wave_geom<BOUNDED>(W, nl, lane);

    for (int t = 0; t < samples; t++) {
        for (int64_t g = 0; g < every; g++) wave_generation<NW, RPL, BOUNDED>(w, geom, rule);
        if (TRACE) {
            // (wave_population, inline for the same reason: all 96 TRACE kernels)
            // lanes past the last active one hold whatever the arithmetic left there: they count as 0
            uint32_t pop = 0;
#pragma unroll
            for (int i = 0; i < RPL; i++)
#pragma unroll
                for (int j = 0; j < NW; j++) pop += __popc(w[i][j]);
            pop = wave_sum_u32(active ? pop : 0u);
            if (lane == 0) trace[(int64_t)t * count + board] = pop;
        }
    }

    if (!active) return;
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) rows[i * NW + j] = w[i][j];
}

// The same under a Generations rule of P decay planes (gol_batch_wave.h): the rule one packed word, or a table of one
// per board where `rules` is not null; trace != nullptr: after each `every` generations the number of state-1 cells goes
// to trace[t * count + board], otherwise samples is 1.  One kernel per (NW, RPL, boundary, P): nstates, the rule's
// source and the trace are run-time tests.
template <int NW, int RPL, bool BOUNDED, int P>
__global__ __launch_bounds__(256) void gol_gen_step(uint32_t* __restrict__ words, int64_t plane_stride, int64_t count,
                                                    int W, int H, int samples, int64_t every,
                                                    uint32_t* __restrict__ trace, uint32_t rule,
                                                    const uint32_t* __restrict__ rules, int nstates) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t board = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (board >= count) return;
    const int nl = H / RPL;  // active lanes
    const bool active = lane < nl;
    BoardWave<RuleTable> gw;
    gw.geom = wave_geom<BOUNDED>(W, nl, lane);
    gw.rule = board_rule(board, rule, rules);
    gw.masks = gen_masks(nstates);
    gw.lanes = 0;  // (the census's)
    uint32_t* rows = words + (board * H + lane * RPL) * NW;  // (an inactive lane's points past its board: never used)
    BoardRegs<NW, RPL, P> b;
    board_load(b, rows, plane_stride, active);

    for (int t = 0; t < samples; t++) {
        for (int64_t g = 0; g < every; g++) board_generation<NW, RPL, BOUNDED, P>(b, gw);
        if (trace) {
            const uint32_t pop = wave_population(b.a, active);
            if (lane == 0) trace[(int64_t)t * count + board] = pop;
        }
    }

    if (!active) return;
#pragma unroll
    for (int i = 0; i < RPL; i++)
#pragma unroll
        for (int j = 0; j < NW; j++) {
            rows[i * NW + j] = b.a[i][j];
#pragma unroll
            for (int k = 0; k < P; k++) rows[(k + 1) * plane_stride + i * NW + j] = b.d[k][i][j];
        }
}

// One wave per board: out[2 i] = state-1 cells of board i, out[2 i + 1] = the canonical hash partial sum of its stacked
// board: width W, (nstates - 1) H rows, rows [(k - 1) H, k H) the indicator of state k (the board hash's definition on
// 64-cell chunks, DESIGN.md: chunk j of row y has key y * ceil(W / 64) + j, from 0 for each board, running on through
// the states; gol_hash_finalize(partial, W, (nstates - 1) H) on the host makes it the hash of a single board with
// these cells).  At 2 states that is the board itself.
__global__ __launch_bounds__(256) void gol_batch_observe(const uint32_t* __restrict__ words, int64_t plane_stride,
                                                         int64_t count, int W, int H, int nstates,
                                                         unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t board = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (board >= count) return;
    const int nw = (W + 31) / 32, nc = (W + 63) / 64, planes = gen_planes(nstates);
    const uint32_t* b = words + board * H * nw;
    const auto state_word = [&](int idx, int k) {
        const uint32_t* p = b + idx;
        return gen_state_word(p[0], [&](int q) { return p[(q + 1) * plane_stride]; }, planes, k);
    };
    uint64_t pop = 0, sum = 0;
    for (int k = 1; k < nstates; k++)
        for (int idx = lane; idx < nc * H; idx += 64) {
            const int j = idx % nc, y = idx / nc;
            const uint64_t lo = state_word(y * nw + 2 * j, k);
            const uint64_t hi = 2 * j + 1 < nw ? state_word(y * nw + 2 * j + 1, k) : 0u;
            const uint64_t v = lo | (hi << 32);
            if (k == 1) pop += __popcll(v);
            sum += fmix64(v ^ fmix64((uint64_t)((k - 1) * nc * H + idx) + 0x9E3779B97F4A7C15ULL));
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        pop += __shfl_down(pop, off, 64);
        sum += __shfl_down(sum, off, 64);
    }
    if (lane == 0) {
        out[2 * board] = pop;
        out[2 * board + 1] = sum;
    }
}

// bytes -> planes, one thread per word: `rows` rows of W cells (boards back to back are simply more rows).  states: a
// byte is its cell's state, below nstates (checked on the host), so d = s - 1 fits the planes.  Otherwise a byte that is
// not zero is an alive cell, whatever its value, and every decay word is written as zero.
__global__ void gol_batch_pack(const uint8_t* __restrict__ bytes, uint32_t* __restrict__ words, int64_t plane_stride,
                               int W, int nw, int64_t rows, int planes, bool states) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * nw) return;
    const int64_t r = idx / nw;
    const int j = (int)(idx % nw);
    const uint8_t* src = bytes + r * W + 32 * j;
    const int n = W - 32 * j < 32 ? W - 32 * j : 32;
    uint32_t a = 0, d[kGenPlanesMax] = {0, 0, 0};
    for (int b = 0; b < n; b++) {
        const uint32_t s = src[b];
        a |= (uint32_t)(states ? s == 1 : s != 0) << b;
        const uint32_t v = states && s >= 2 ? s - 1 : 0;
#pragma unroll
        for (int q = 0; q < kGenPlanesMax; q++) d[q] |= (v >> q & 1u) << b;
    }
    words[idx] = a;
#pragma unroll
    for (int q = 0; q < kGenPlanesMax; q++)
        if (q < planes) words[idx + (q + 1) * plane_stride] = d[q];
}

// planes -> bytes, one thread per cell, to out[x + r * stride]: the cell's state where `states`, otherwise
// alive ? value : 0 (a dying cell is 0)
__global__ void gol_batch_unpack(const uint32_t* __restrict__ words, int64_t plane_stride, uint8_t* __restrict__ out,
                                 int W, int nw, int64_t rows, int64_t stride, uint8_t value, int planes, bool states) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * W) return;
    const int64_t r = idx / W;
    const int x = (int)(idx % W);
    const uint32_t* p = words + r * nw + (x >> 5);
    uint32_t v = 0;
    if (states)
        for (int q = 0; q < planes; q++) v |= ((p[(q + 1) * plane_stride] >> (x & 31)) & 1u) << q;
    out[x + r * stride] = ((p[0] >> (x & 31)) & 1u) ? (states ? (uint8_t)1 : value) : v ? (uint8_t)(v + 1) : (uint8_t)0;
}

// board i <- gol_seed_splitmix(seed + i): word j of row y = low32(splitmix64((seed + i) ^ (y * nw + j))), cut at W
__global__ void gol_batch_splitmix(uint32_t* __restrict__ words, int64_t count, int W, int H, int nw, uint64_t seed) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)H * nw;
    if (idx >= count * per) return;
    const int64_t board = idx / per, k = idx % per;
    const int j = (int)(k % nw);
    uint32_t v = (uint32_t)splitmix64((seed + (uint64_t)board) ^ (uint64_t)k);
    if (j == nw - 1 && (W & 31)) v &= (1u << (W & 31)) - 1u;
    words[idx] = v;
}

unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_batch_step(uint32_t* words, int64_t count, int64_t W, int64_t H, bool bounded, int64_t samples,
                             int64_t every, uint32_t* trace, int group_waves, uint32_t rule, bool force_table,
                             const uint32_t* rules, int nstates, hipStream_t s) {
    const int rpl = wave_resident_rpl(W, H);
    if (!rpl || !rule_packed_ok(rule) || !words || count < 1 || count > kBatchCountMax || samples < 1 ||
        samples > INT32_MAX || every < 1 || (!trace && samples != 1) || (group_waves != 1 && group_waves != 4) ||
        !gen_states_ok(nstates))
        return hipErrorInvalidValue;
    const dim3 grid(blocks(count, group_waves)), block(64 * group_waves);
    const int w = (int)W, h = (int)H, n = (int)samples, nw = (int)((W + 31) / 32);
    if (nstates > 2)
        return dispatch_planes(gen_planes(nstates), [&](auto P) {
            return wave_dispatch(
                [&](auto NW, auto RPL, auto B) {
                    hipLaunchKernelGGL((gol_gen_step<NW, RPL, B, P>), grid, block, 0, s, words, count * H * nw, count, w,
                                       h, n, every, trace, rule, rules, nstates);
                    return hipGetLastError();
                },
                nw, rpl, bounded);
        });
    const auto launch = [&](auto NW, auto RPL, auto B, auto T) {
        switch (rule_family(rule, force_table, rules)) {
            case RuleFamily::Life:
                hipLaunchKernelGGL((gol_batch_step<NW, RPL, B, T>), grid, block, 0, s, words, count, w, h, n, every,
                                   trace);
                break;
            case RuleFamily::Table:
                hipLaunchKernelGGL((gol_batch_step<NW, RPL, B, T, uint32_t>), grid, block, 0, s, words, count, w, h, n,
                                   every, trace, rule);
                break;
            case RuleFamily::PerBoard:
                hipLaunchKernelGGL((gol_batch_step<NW, RPL, B, T, const uint32_t*>), grid, block, 0, s, words, count, w,
                                   h, n, every, trace, rules);
                break;
        }
        return hipGetLastError();
    };
    return wave_dispatch(launch, nw, rpl, bounded, trace != nullptr);
}

hipError_t launch_batch_observe(const uint32_t* words, int64_t plane_stride, int64_t count, int64_t W, int64_t H,
                                int nstates, unsigned long long* out, hipStream_t s) {
    if (!wave_resident_rpl(W, H) || !words || !out || count < 1 || count > kBatchCountMax || !gen_states_ok(nstates) ||
        plane_stride < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gol_batch_observe, dim3(blocks(count, 4)), dim3(256), 0, s, words, plane_stride, count, (int)W,
                       (int)H, nstates, out);
    return hipGetLastError();
}

// rows <= 2^30 keeps both grids below 2^31 workgroups
hipError_t launch_batch_pack(const uint8_t* bytes, uint32_t* words, int64_t plane_stride, int64_t W, int64_t rows,
                             int nstates, bool states, hipStream_t s) {
    if (W < 1 || W > 128 || rows < 1 || rows > ((int64_t)1 << 30) || !gen_states_ok(nstates) || plane_stride < 1)
        return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    hipLaunchKernelGGL(gol_batch_pack, dim3(blocks(rows * nw, 256)), dim3(256), 0, s, bytes, words, plane_stride, (int)W,
                       nw, rows, gen_planes(nstates), states);
    return hipGetLastError();
}

hipError_t launch_batch_unpack(const uint32_t* words, int64_t plane_stride, uint8_t* out, int64_t W, int64_t rows,
                               int64_t stride, uint8_t value, int nstates, bool states, hipStream_t s) {
    if (W < 1 || W > 128 || rows < 1 || rows > ((int64_t)1 << 30) || stride < W || !gen_states_ok(nstates) ||
        plane_stride < 1)
        return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    hipLaunchKernelGGL(gol_batch_unpack, dim3(blocks(rows * W, 256)), dim3(256), 0, s, words, plane_stride, out, (int)W,
                       nw, rows, stride, value, gen_planes(nstates), states);
    return hipGetLastError();
}

hipError_t launch_batch_splitmix(uint32_t* words, int64_t count, int64_t W, int64_t H, uint64_t seed, hipStream_t s) {
    if (!wave_resident_rpl(W, H) || count < 1 || count > kBatchCountMax) return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    hipLaunchKernelGGL(gol_batch_splitmix, dim3(blocks(count * H * nw, 256)), dim3(256), 0, s, words, count, (int)W,
                       (int)H, nw, seed);
    return hipGetLastError();
}

}  // namespace gol
