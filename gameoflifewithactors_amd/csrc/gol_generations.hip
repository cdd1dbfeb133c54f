// gol_generations.hip -- Generations rules (B/S/C, gol_generations.h) on a batch of small boards: step, population
// trace, cycle census, the stacked observables and state bytes, one wavefront per board (gfx950).
//
// Storage.  The alive plane is the batch's `words` as gol_batch.hip lays it out (boards back to back, board i row y = NW
// words at words[(i * H + y) * NW], bits at or beyond W zero), so pack, unpack, splitmix and every 2-state kernel keep
// working on it.  Decay plane k (0 .. P - 1, P = gen_planes(nstates)) is a whole further array of the same shape at
// words + (k + 1) * plane_stride, plane_stride = count * H * NW words: a cell's word sits at the same index in every
// plane.  A dying cell in state s holds d = s - 1 as a binary number, bit k in plane k; a dead or alive cell holds 0.
//
// Geometry: gol_wave_body.h's (lane L holds rows L*RPL .., NW words each, wave_dispatch picks NW and RPL).  The alive
// plane advances through wave_generation's rule-table arm unchanged -- only state-1 cells are neighbours -- and the
// decay planes by gen_decay, per word, with no cross-lane traffic.  nstates is a kernel argument (P scalar masks), the
// rule one packed word or a table of one per board (a null test and one scalar load per wave), the trace a null test:
// one step kernel and one census kernel per (NW, RPL, boundary, P).
//
// Invariants.  Pad bits: wave_generation cuts the alive plane's last word (lastmask) before gen_decay sees it, and
// gen_decay keeps a bit zero in every plane where the old alive plane and the old decay planes had it zero.  Lanes at
// or beyond nl load zeros, run the same instructions on whatever the row exchange leaves them, are read by no active
// lane (wave_geom's addresses), count for nothing (`active` in the population, `lanes` in the census) and are never
// stored.  Rows outside a bounded board contribute nothing: up_mask / dn_mask in wave_generation, and the decay needs
// no neighbour.
#include "gol_batch_host.h"
#include "gol_cycle_search.h"
#include "gol_generations.h"
#include "gol_internal.h"
#include "gol_rule.h"
#include "gol_wave_body.h"
#include "gol_wave_dispatch.h"

namespace gol {
namespace {

// One board in one wave's registers: the alive plane and P decay planes.
template <int NW, int RPL, int P>
struct GenBoard {
    uint32_t a[RPL][NW];
    uint32_t d[P][RPL][NW];
};

// What a wave needs beside its board.
struct GenWave {
    WaveGeom geom;
    RuleTable rule;
    GenMasks masks;
    uint64_t lanes;  // the lanes that hold rows of the board
};

// The wave's rule: the launch's one packed word, or its board's entry of the table (one scalar load).
__device__ __forceinline__ RuleTable gen_rule(int64_t board, uint32_t rule, const uint32_t* rules) {
    return rules ? board_rule(board, rules) : RuleTable{rule};
}

template <int NW, int RPL, int P>
__device__ __forceinline__ void gen_load(GenBoard<NW, RPL, P>& b, const uint32_t* rows, int64_t plane_stride,
                                         bool active) {
    wave_load_rows(b.a, rows, active);
#pragma unroll
    for (int k = 0; k < P; k++) wave_load_rows(b.d[k], rows + (k + 1) * plane_stride, active);
}

// One synchronous generation of the wave's board, in place.
template <int NW, int RPL, bool BOUNDED, int P>
__device__ __forceinline__ void gen_generation(GenBoard<NW, RPL, P>& b, const GenWave& w) {
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

// Board `blockIdx.x * waves per group + wave` runs `samples` x `every` generations in registers.  trace != nullptr:
// after each `every` generations the number of state-1 cells goes to trace[t * count + board]; otherwise samples is 1.
// A wave past the last board leaves before it touches memory.
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
    GenWave gw;
    gw.geom = wave_geom<BOUNDED>(W, nl, lane);
    gw.rule = gen_rule(board, rule, rules);
    gw.masks = gen_masks(nstates);
    gw.lanes = 0;
    uint32_t* rows = words + (board * H + lane * RPL) * NW;  // (an inactive lane's points past its board: never used)
    GenBoard<NW, RPL, P> b;
    gen_load(b, rows, plane_stride, active);

    for (int t = 0; t < samples; t++) {
        for (int64_t g = 0; g < every; g++) gen_generation<NW, RPL, BOUNDED, P>(b, gw);
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

// The census's state type (gol_cycle_search.h): gol_cycles.hip's, with 1 + P planes and `equal` over all of them.
template <int NW, int RPL, bool BOUNDED, int P>
struct GenCycleBoard {
    GenBoard<NW, RPL, P> b;
    const GenWave* wave;

    __device__ __forceinline__ void step() { gen_generation<NW, RPL, BOUNDED, P>(b, *wave); }
    __device__ __forceinline__ bool equal(const GenCycleBoard& o) const {
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < RPL; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) {
                diff = lut3<0xBE>(diff, b.a[i][j], o.b.a[i][j]);  // d | (a ^ b)
#pragma unroll
                for (int k = 0; k < P; k++) diff = lut3<0xBE>(diff, b.d[k][i][j], o.b.d[k][i][j]);
            }
        return (__ballot(diff != 0) & wave->lanes) == 0;
    }
};

// Board blockIdx.x: out[4 board ..] = transient, period, state-1 cells of B_transient, generation steps run.  Read-only.
template <int NW, int RPL, bool BOUNDED, int P>
__global__ __launch_bounds__(64) void gol_gen_cycles(const uint32_t* __restrict__ words, int64_t plane_stride,
                                                     int64_t count, int W, int H, int max_generations,
                                                     int32_t* __restrict__ out, uint32_t rule,
                                                     const uint32_t* __restrict__ rules, int nstates) {
    const int lane = threadIdx.x;
    const int64_t board = blockIdx.x;
    if (board >= count) return;
    const int nl = H / RPL;
    const bool active = lane < nl;
    const uint32_t* rows = words + (board * H + lane * RPL) * NW;
    GenWave gw;
    gw.geom = wave_geom<BOUNDED>(W, nl, lane);
    gw.rule = gen_rule(board, rule, rules);
    gw.masks = gen_masks(nstates);
    gw.lanes = __ballot(active);
    using Board = GenCycleBoard<NW, RPL, BOUNDED, P>;
    const auto load = [&]() {
        Board s;
        s.wave = &gw;
        gen_load(s.b, rows, plane_stride, active);
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

__device__ __forceinline__ uint64_t mix64(uint64_t k) {  // the hash's fmix64 (gol_formats.hip)
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// One wave per board: out[2 i] = state-1 cells of board i, out[2 i + 1] = the canonical hash partial sum of the stacked
// board: width W, (nstates - 1) H rows, rows [(k - 1) H, k H) the indicator of state k (gol_batch.hip's observe with
// the chunk keys running on through the states; gol_hash_finalize(partial, W, (nstates - 1) H) on the host).
__global__ __launch_bounds__(256) void gol_gen_observe(const uint32_t* __restrict__ words, int64_t plane_stride,
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
            sum += mix64(v ^ mix64((uint64_t)((k - 1) * nc * H + idx) + 0x9E3779B97F4A7C15ULL));
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

// state bytes -> planes, one thread per word: `rows` rows of W cells.  The bytes are below nstates (checked on the
// host), so d = s - 1 fits the planes.
__global__ void gol_gen_pack(const uint8_t* __restrict__ states, uint32_t* __restrict__ words, int64_t plane_stride,
                             int W, int nw, int64_t rows, int planes) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * nw) return;
    const int64_t r = idx / nw;
    const int j = (int)(idx % nw);
    const uint8_t* src = states + r * W + 32 * j;
    const int n = W - 32 * j < 32 ? W - 32 * j : 32;
    uint32_t a = 0, d[kGenPlanesMax] = {0, 0, 0};
    for (int b = 0; b < n; b++) {
        const uint32_t s = src[b];
        a |= (uint32_t)(s == 1) << b;
        const uint32_t v = s >= 2 ? s - 1 : 0;
#pragma unroll
        for (int q = 0; q < kGenPlanesMax; q++) d[q] |= (v >> q & 1u) << b;
    }
    words[idx] = a;
#pragma unroll
    for (int q = 0; q < kGenPlanesMax; q++)
        if (q < planes) words[idx + (q + 1) * plane_stride] = d[q];
}

// planes -> state bytes, one thread per cell
__global__ void gol_gen_unpack(const uint32_t* __restrict__ words, int64_t plane_stride, uint8_t* __restrict__ out,
                               int W, int nw, int64_t rows, int planes) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * W) return;
    const int64_t r = idx / W;
    const int x = (int)(idx % W);
    const uint32_t* p = words + r * nw + (x >> 5);
    uint32_t v = 0;
    for (int q = 0; q < planes; q++) v |= ((p[(q + 1) * plane_stride] >> (x & 31)) & 1u) << q;
    out[idx] = ((p[0] >> (x & 31)) & 1u) ? 1 : v ? (uint8_t)(v + 1) : 0;
}

unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <class F>
hipError_t dispatch_planes(int planes, F&& f) {
    switch (planes) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_gen_step(uint32_t* words, int64_t count, int64_t W, int64_t H, bool bounded, int64_t samples,
                           int64_t every, uint32_t* trace, int group_waves, uint32_t rule, const uint32_t* rules,
                           int nstates, hipStream_t s) {
    const int rpl = wave_resident_rpl(W, H);
    if (!rpl || !rule_packed_ok(rule) || !words || count < 1 || count > kBatchCountMax || samples < 1 ||
        samples > INT32_MAX || every < 1 || (!trace && samples != 1) || (group_waves != 1 && group_waves != 4) ||
        !gen_states_ok(nstates))
        return hipErrorInvalidValue;
    const dim3 grid(blocks(count, group_waves)), block(64 * group_waves);
    const int w = (int)W, h = (int)H, n = (int)samples, nw = (int)((W + 31) / 32);
    const int64_t stride = count * H * nw;
    return dispatch_planes(gen_planes(nstates), [&](auto P) {
        return wave_dispatch(
            [&](auto NW, auto RPL, auto B) {
                hipLaunchKernelGGL((gol_gen_step<NW, RPL, B, P>), grid, block, 0, s, words, stride, count, w, h, n,
                                   every, trace, rule, rules, nstates);
                return hipGetLastError();
            },
            nw, rpl, bounded);
    });
}

hipError_t launch_gen_cycles(const uint32_t* words, int64_t count, int64_t W, int64_t H, bool bounded,
                             int64_t max_generations, int32_t* out, uint32_t rule, const uint32_t* rules, int nstates,
                             hipStream_t s) {
    const int rpl = wave_resident_rpl(W, H);
    if (!rpl || !rule_packed_ok(rule) || !words || !out || count < 1 || count > kBatchCountMax ||
        max_generations < 1 || max_generations > kCycleGenerationsMax || !gen_states_ok(nstates))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)count), block(64);  // count <= 2^22
    const int w = (int)W, h = (int)H, G = (int)max_generations, nw = (int)((W + 31) / 32);
    const int64_t stride = count * H * nw;
    return dispatch_planes(gen_planes(nstates), [&](auto P) {
        return wave_dispatch(
            [&](auto NW, auto RPL, auto B) {
                hipLaunchKernelGGL((gol_gen_cycles<NW, RPL, B, P>), grid, block, 0, s, words, stride, count, w, h, G,
                                   out, rule, rules, nstates);
                return hipGetLastError();
            },
            nw, rpl, bounded);
    });
}

hipError_t launch_gen_observe(const uint32_t* words, int64_t count, int64_t W, int64_t H, int nstates,
                              unsigned long long* out, hipStream_t s) {
    if (!wave_resident_rpl(W, H) || !words || !out || count < 1 || count > kBatchCountMax || !gen_states_ok(nstates))
        return hipErrorInvalidValue;
    const int64_t stride = count * H * ((W + 31) / 32);
    hipLaunchKernelGGL(gol_gen_observe, dim3(blocks(count, 4)), dim3(256), 0, s, words, stride, count, (int)W, (int)H,
                       nstates, out);
    return hipGetLastError();
}

// rows <= 2^30 keeps both grids below 2^31 workgroups
hipError_t launch_gen_pack(const uint8_t* states, uint32_t* words, int64_t plane_stride, int64_t W, int64_t rows,
                           int nstates, hipStream_t s) {
    if (W < 1 || W > 128 || rows < 1 || rows > ((int64_t)1 << 30) || !gen_states_ok(nstates) || plane_stride < 1)
        return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    hipLaunchKernelGGL(gol_gen_pack, dim3(blocks(rows * nw, 256)), dim3(256), 0, s, states, words, plane_stride, (int)W,
                       nw, rows, gen_planes(nstates));
    return hipGetLastError();
}

hipError_t launch_gen_unpack(const uint32_t* words, int64_t plane_stride, uint8_t* out, int64_t W, int64_t rows,
                             int nstates, hipStream_t s) {
    if (W < 1 || W > 128 || rows < 1 || rows > ((int64_t)1 << 30) || !gen_states_ok(nstates) || plane_stride < 1)
        return hipErrorInvalidValue;
    const int nw = (int)((W + 31) / 32);
    hipLaunchKernelGGL(gol_gen_unpack, dim3(blocks(rows * W, 256)), dim3(256), 0, s, words, plane_stride, out, (int)W,
                       nw, rows, gen_planes(nstates));
    return hipGetLastError();
}

}  // namespace gol
