// gol_rule_step.hip -- the rule-generic streaming pass: K generations of ANY life-like rule (gol_rule.h) per pass over a
// packed board of any size, on the board's own ping-pong buffers and layout (gol_layout.h).  gol_step runs it on packed
// boards whose rule is not B3/S23 (gol_policy.cpp choose_pass); the B3/S23 passes are other files and other kernels.
//
// The simple form of gol_stream_step (gol_step.hip), geometry and safety argument in gol_rule_plan.h:
//   - one wavefront per column strip of 64 blocks (lane i <-> block first - 1 + i; lanes 0 and 63 are halo, 62 stored)
//     and row segment (seg rows stored, seg + 2 K streamed);
//   - block-edge words by DPP wave_shr:1 / wave_shl:1 (zero into the wave's outer lanes: an error that starts at a halo
//     lane's outer edge moves one cell per generation, K <= 8 cells into a block of >= 32);
//   - per level a 3-row window of row sums (row_sum_block) and the centre row.  The window's three slots rotate by
//     static index over a loop trip of three rows, so no row is ever moved between registers: 5 K M words are live
//     from one step to the next (two rows of sums and one of words per level);
//   - every output row finished by rule_row<M> below (rule_next_row's arithmetic, gol_bitlogic.h: 9 fixed + 2 per set
//     rule bit v_bitop3 per word, the rule one scalar kernel argument tested bit by bit by scalar branches);
//   - a scheduling barrier between levels;
//   - the next trip's three rows are loaded at the top of a trip.
// A level's first outputs are computed from a window that is not full yet (zeros); they are what the rows K above the
// segment would cost anyway, and nothing that is stored depends on them: the last level's output at step t is row
// r0 - 2 K + t, stored from t = 2 K, and it depends on level l's outputs from step 2 l + 2 on, the first with three
// loaded rows behind it.
//
// Torus: every lane loads block index mod blocks-per-row and row index mod H.  Bounded: blocks and rows outside the
// board load nothing (zero) and are forced dead at EVERY level -- under a rule with birth bit 0 a dead cell with no
// live neighbour comes alive, outside the board too, unless it is masked.
//
// gol_rule_stream_ragged below is the same pass on the whole-word scratch rows of a ragged byte board (width not a
// multiple of 32; gol_policy.cpp use_rule_ragged).
#include "gol_internal.h"
#include "gol_bitlogic.h"
#include "gol_layout.h"
#include "gol_rule.h"
#include "gol_rule_plan.h"

namespace gol {
namespace {

__device__ __forceinline__ uint32_t lane_left(uint32_t v) {  // lane i <- lane i - 1, 0 into lane 0
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x138, 0xf, 0xf, true);  // wave_shr:1
}
__device__ __forceinline__ uint32_t lane_right(uint32_t v) {  // lane i <- lane i + 1, 0 into lane 63
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xf, 0xf, true);  // wave_shl:1
}

template <int M>
__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&v)[M]) {
    if constexpr (M == 1) {
        v[0] = *p;
    } else if constexpr (M == 2) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        v[0] = t.x, v[1] = t.y;
    } else {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
}
template <int M>
__device__ __forceinline__ void store_words(uint32_t* p, const uint32_t (&v)[M]) {
    if constexpr (M == 1)
        *p = v[0];
    else if constexpr (M == 2)
        *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
    else
        *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
}

// rule_next_row (gol_bitlogic.h) for this kernel: the same planes and the same terms (rule_term / rule_term_high), but
// every rule-bit test is kept a scalar branch.  Left to itself the compiler turns the tests of a row of one or two
// words into selects -- all 18 terms computed for every rule, 3 instructions each -- where a branch costs a clear bit
// nothing; an empty volatile statement inside a term cannot be executed speculatively, so the branch stays.
template <int N>
__device__ __forceinline__ void rule_row(const uint32_t (&sP)[N], const uint32_t (&cP)[N], const uint32_t (&sC)[N],
                                         const uint32_t (&cC)[N], const uint32_t (&sN)[N], const uint32_t (&cN)[N],
                                         const uint32_t (&alive)[N], uint32_t rule, uint32_t (&out)[N]) {
    uint32_t t0[N], t1[N], t2[N], t3[N], qd[N], qa[N], acc[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t B = lut3<0xE8>(sP[j], sC[j], sN[j]);
        const uint32_t X = lut3<0x96>(cP[j], cC[j], cN[j]);
        const uint32_t Y = lut3<0xE8>(cP[j], cC[j], cN[j]);
        t0[j] = lut3<0x96>(sP[j], sC[j], sN[j]);
        t1[j] = B ^ X;
        t2[j] = lut3<0x78>(B, X, Y);
        t3[j] = lut3<0x80>(B, X, Y);
        qd[j] = ~(t3[j] | alive[j]);
        qa[j] = alive[j] & ~t3[j];
        acc[j] = 0;
    }
    asm volatile("" : "+s"(rule));
#define GOL_RULE_BIT(n, term) \
    if (rule >> n & 1) {      \
        asm volatile("");     \
        term;                 \
    }
    GOL_RULE_BIT(0, (rule_term<0, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(1, (rule_term<1, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(2, (rule_term<2, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(3, (rule_term<3, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(4, (rule_term<4, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(5, (rule_term<5, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(6, (rule_term<6, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(7, (rule_term<7, false>(acc, t0, t1, t2, qd)))
    GOL_RULE_BIT(8, (rule_term_high<0x02>(acc, t3, t0, alive)))
    GOL_RULE_BIT(9, (rule_term<1, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(10, (rule_term<2, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(11, (rule_term<3, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(12, (rule_term<4, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(13, (rule_term<5, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(14, (rule_term<6, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(15, (rule_term<7, true>(acc, t0, t1, t2, qa)))
    GOL_RULE_BIT(16, (rule_term_high<0x20>(acc, t3, t0, alive)))
    GOL_RULE_BIT(17, (rule_term_high<0x80>(acc, t3, t0, alive)))
#undef GOL_RULE_BIT
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = acc[j];
}

// The K windows of one wave.  Slot t % 3 of a level takes the row that enters it at step t.
template <int K, int M, bool BOUNDED>
struct RuleWindows {
    uint32_t s[K][3][M], c[K][3][M], a[K][3][M];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int l = 0; l < K; l++)
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int j = 0; j < M; j++) s[l][p][j] = c[l][p][j] = a[l][p][j] = 0;
    }

    // One step: row x (generation 0) enters level 0, and every level hands the row it finishes to the next; x leaves as
    // the last level's output.  yo: the row level 0 finishes at this step (bounded boards: level l finishes yo - l).
    template <int PH>
    __device__ __forceinline__ void step(uint32_t (&x)[M], uint32_t rule, uint32_t lanemask, int64_t yo, int64_t H) {
        constexpr int P = (PH + 1) % 3, C = (PH + 2) % 3;
#pragma unroll
        for (int l = 0; l < K; l++) {
            const uint32_t lft = lane_left(x[M - 1]);
            const uint32_t rgt = lane_right(x[0]);
            row_sum_block<M>(x, lft, rgt, s[l][PH], c[l][PH]);
#pragma unroll
            for (int j = 0; j < M; j++) a[l][PH][j] = x[j];
            rule_row<M>(s[l][P], c[l][P], s[l][C], c[l][C], s[l][PH], c[l][PH], a[l][C], rule, x);
            if constexpr (BOUNDED) {
                const int64_t y = yo - l;
                const uint32_t m = (y >= 0 && y < H) ? lanemask : 0u;
#pragma unroll
                for (int j = 0; j < M; j++) x[j] &= m;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

template <int K, int M, bool BOUNDED>
__global__ __launch_bounds__(64 * kRuleWavesPerBlock) void gol_rule_stream(const uint32_t* __restrict__ src,
                                                                           uint32_t* __restrict__ dst, RulePlan plan,
                                                                           int64_t pitch, uint32_t rule) {
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kRuleWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= plan.nwaves) return;
    const RuleWave w = rule_wave(plan, wave);
    int64_t lblk, sblk;
    const bool lane_ld = rule_lane_load(plan, w, lane, &lblk) || !BOUNDED;  // (a torus lane always loads)
    const bool lane_st = rule_lane_store(plan, w, lane, &sblk);
    const uint32_t lanemask = lane_ld ? 0xffffffffu : 0u;
    const int64_t H = plan.H;
    const int64_t ybase = w.r0 - K;  // the row step 0 loads, before the modulo

    // step t's row: loaded only inside the stream, (bounded) inside the board and by lanes inside the board
    int64_t ywrap = BOUNDED ? ybase : rule_mod(ybase, H);  // the next row to load (torus: wrapped)
    auto load_row = [&](int64_t t, uint32_t (&v)[M]) {
#pragma unroll
        for (int j = 0; j < M; j++) v[j] = 0;
        const bool row_ok = t < w.steps && (!BOUNDED || (ywrap >= 0 && ywrap < H));
        if (row_ok && lane_ld) load_words<M>(src + ywrap * pitch + lblk * M, v);
        ywrap++;
        if (!BOUNDED && ywrap == H) ywrap = 0;
    };

    RuleWindows<K, M, BOUNDED> win;
    win.clear();
    uint32_t nxt[kRuleTripRows][M];
#pragma unroll
    for (int r = 0; r < kRuleTripRows; r++) load_row(r, nxt[r]);

    const int64_t nstore = w.r1 - w.r0;
#pragma nounroll
    for (int64_t T = 0; T < w.trips; T++) {
        uint32_t cur[kRuleTripRows][M];
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++)
#pragma unroll
            for (int j = 0; j < M; j++) cur[r][j] = nxt[r][j];
        const int64_t t0 = T * kRuleTripRows;
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++) load_row(t0 + kRuleTripRows + r, nxt[r]);
        __builtin_amdgcn_sched_barrier(0);  // the prefetch stays at the top of the trip
        auto finish = [&](int64_t t, uint32_t (&x)[M]) {  // the last level's output of step t is row r0 - 2 K + t
            const int64_t o = t - 2 * K;
            if (o >= 0 && o < nstore && lane_st) store_words<M>(dst + (w.r0 + o) * pitch + sblk * M, x);
        };
        win.template step<0>(cur[0], rule, lanemask, ybase + t0 - 1, H);
        finish(t0, cur[0]);
        win.template step<1>(cur[1], rule, lanemask, ybase + t0, H);
        finish(t0 + 1, cur[1]);
        win.template step<2>(cur[2], rule, lanemask, ybase + t0 + 1, H);
        finish(t0 + 2, cur[2]);
    }
}

// gol_rule_stream at M = 1 on the scratch rows of a ragged byte board W cells wide: rows of plan.nblocks = pitch =
// ceil(W / 32) words, the last one partial with zero pad bits (gol_rule_plan.h "Ragged rows").  Only what
// a lane loads, the level mask of the partial word's lane and what that lane stores differ; the windows, the DPP edges
// and the levels do not know.  Torus: a lane whose 32 ring cells are not one whole word of the row assembles them from
// up to three (rule_ragged_load), and only in the waves that hold such a lane -- `shifted` is wave-uniform, so every
// other wave of a wide board runs the aligned pass's one load per row.  A kernel of its own beside gol_rule_stream, not
// a template value of it: a body shared through a function changed how the compiler reads the plan out of the kernel
// arguments, in every instantiation of the aligned kernel.
template <int K, bool BOUNDED>
__global__ __launch_bounds__(64 * kRuleWavesPerBlock) void gol_rule_stream_ragged(const uint32_t* __restrict__ src,
                                                                                  uint32_t* __restrict__ dst,
                                                                                  RulePlan plan, int64_t pitch,
                                                                                  uint32_t rule, int64_t W) {
    constexpr int M = 1;
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kRuleWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= plan.nwaves) return;
    const RuleWave w = rule_wave(plan, wave);
    int64_t lblk, sblk;
    const bool lane_ld = rule_lane_load(plan, w, lane, &lblk) || !BOUNDED;  // (a torus lane always loads)
    const bool lane_st = rule_lane_store(plan, w, lane, &sblk);
    // bounded: the cells of the lane's word that may live; torus: the lane's window on the ring of W cells
    const uint32_t lanemask = BOUNDED ? rule_ragged_level_mask(plan, w, lane, W) : 0xffffffffu;
    const uint32_t stmask = rule_ragged_store_mask(plan, w, lane, W);
    RaggedWindow rw{};     // torus only: the lane's window, and whether any lane of this wave assembles its word
    bool shifted = false;  // (wave-uniform)
    if constexpr (!BOUNDED) {
        rw = rule_ragged_window(w, lane, W);
        shifted = __ballot(!rule_ragged_plain(rw)) != 0;
    }
    const int64_t H = plan.H;
    const int64_t ybase = w.r0 - K;  // the row step 0 loads, before the modulo

    // step t's row: loaded only inside the stream, (bounded) inside the board and by lanes inside the board
    int64_t ywrap = BOUNDED ? ybase : rule_mod(ybase, H);  // the next row to load (torus: wrapped)
    auto load_row = [&](int64_t t, uint32_t (&v)[M]) {
#pragma unroll
        for (int j = 0; j < M; j++) v[j] = 0;
        const bool row_ok = t < w.steps && (!BOUNDED || (ywrap >= 0 && ywrap < H));
        if constexpr (BOUNDED) {
            if (row_ok && lane_ld) v[0] = src[ywrap * pitch + lblk];
        } else {
            if (row_ok) v[0] = shifted ? rule_ragged_load(src + ywrap * pitch, rw) : src[ywrap * pitch + rw.word];
        }
        ywrap++;
        if (!BOUNDED && ywrap == H) ywrap = 0;
    };

    RuleWindows<K, M, BOUNDED> win;
    win.clear();
    uint32_t nxt[kRuleTripRows][M];
#pragma unroll
    for (int r = 0; r < kRuleTripRows; r++) load_row(r, nxt[r]);

    const int64_t nstore = w.r1 - w.r0;
#pragma nounroll
    for (int64_t T = 0; T < w.trips; T++) {
        uint32_t cur[kRuleTripRows][M];
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++)
#pragma unroll
            for (int j = 0; j < M; j++) cur[r][j] = nxt[r][j];
        const int64_t t0 = T * kRuleTripRows;
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++) load_row(t0 + kRuleTripRows + r, nxt[r]);
        __builtin_amdgcn_sched_barrier(0);  // the prefetch stays at the top of the trip
        auto finish = [&](int64_t t, uint32_t (&x)[M]) {  // the last level's output of step t is row r0 - 2 K + t
            const int64_t o = t - 2 * K;
            if (o >= 0 && o < nstore && lane_st) dst[(w.r0 + o) * pitch + sblk] = x[0] & stmask;
        };
        win.template step<0>(cur[0], rule, lanemask, ybase + t0 - 1, H);
        finish(t0, cur[0]);
        win.template step<1>(cur[1], rule, lanemask, ybase + t0, H);
        finish(t0 + 1, cur[1]);
        win.template step<2>(cur[2], rule, lanemask, ybase + t0 + 1, H);
        finish(t0 + 2, cur[2]);
    }
}

template <int K>
hipError_t launch_k_ragged(const uint32_t* src, uint32_t* dst, const RulePlan& plan, int64_t W, uint32_t rule,
                           hipStream_t s) {
    const dim3 grid((unsigned)rule_stream_grid(plan)), block(64 * kRuleWavesPerBlock);
    if (plan.bounded)
        hipLaunchKernelGGL((gol_rule_stream_ragged<K, true>), grid, block, 0, s, src, dst, plan, plan.nblocks, rule, W);
    else
        hipLaunchKernelGGL((gol_rule_stream_ragged<K, false>), grid, block, 0, s, src, dst, plan, plan.nblocks, rule, W);
    return hipGetLastError();
}

template <int K, int M>
hipError_t launch_km(const uint32_t* src, uint32_t* dst, const RulePlan& plan, int64_t pitch, uint32_t rule,
                     hipStream_t s) {
    const dim3 grid((unsigned)rule_stream_grid(plan)), block(64 * kRuleWavesPerBlock);
    if (plan.bounded)
        hipLaunchKernelGGL((gol_rule_stream<K, M, true>), grid, block, 0, s, src, dst, plan, pitch, rule);
    else
        hipLaunchKernelGGL((gol_rule_stream<K, M, false>), grid, block, 0, s, src, dst, plan, pitch, rule);
    return hipGetLastError();
}

template <int M>
hipError_t launch_m(const uint32_t* src, uint32_t* dst, const RulePlan& plan, int64_t pitch, uint32_t rule,
                    hipStream_t s) {
    switch (plan.K) {
        case 8: return launch_km<8, M>(src, dst, plan, pitch, rule, s);
        case 4: return launch_km<4, M>(src, dst, plan, pitch, rule, s);
        case 2: return launch_km<2, M>(src, dst, plan, pitch, rule, s);
        case 1: return launch_km<1, M>(src, dst, plan, pitch, rule, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// Depths of the pass: the deepest of 8, 4, 2, 1 that n generations hold (gol_passes.cpp caps n at rule_stream_max_k, so
// a call is n / 4 passes of 4 and then the binary remainder).
int rule_stream_largest_k(int64_t n) { return n >= 8 ? 8 : (n >= 4 ? 4 : (n >= 2 ? 2 : (n >= 1 ? 1 : 0))); }

// The depth gol_step runs: 4.  The pass is bound by the latency of a wave's dependent chain, not by memory (DESIGN.md
// 4.12), so what counts is waves per SIMD and rows per wave: K = 8 against K = 4 measured 6.8 against 4.8 us per
// generation at 4096^2, 17.4 against 13.8 at 16384^2 and, at M = 4 where K = 8 takes 268 registers (one wave per SIMD),
// 236 against 112 at 65536^2 (profiles/board_rules/probe_depth_segments.txt).  K = 8 stays instantiated and tested
// (debug option "rule_k").
int rule_stream_max_k(int ilv) {
    (void)ilv;
    return 4;
}

RulePlan rule_stream_plan(int64_t W, int64_t H, int ilv, int k, bool bounded, int64_t seg_opt) {
    const int cus = device_cus();
    // 32 waves per CU, a few rounds of what the device holds: short segments measured faster than few recomputed rows at
    // every size (each wave is one dependent chain: profiles/board_rules/probe_depth_segments.txt)
    return rule_plan(W / (32 * (int64_t)ilv), H, k, bounded, seg_opt, cus > 0 ? (int64_t)cus * 32 : 8192);
}

hipError_t launch_rule_stream(const uint32_t* src, uint32_t* dst, int64_t W, int64_t H, int64_t pitch, int ilv, int k,
                              bool bounded, uint32_t rule, int64_t seg_opt, hipStream_t s) {
    if ((ilv != 1 && ilv != 2 && ilv != 4) || W < 32 * ilv || W % (32 * ilv) || H < 1 || pitch < W / 32 || pitch % ilv ||
        !rule_packed_ok(rule) ||rule_stream_largest_k(k) != k)
        return hipErrorInvalidValue;
    const RulePlan plan = rule_stream_plan(W, H, ilv, k, bounded, seg_opt);
    if (rule_stream_grid(plan) > 0x7fffffff) return hipErrorInvalidValue;
    switch (ilv) {
        case 1: return launch_m<1>(src, dst, plan, pitch, rule, s);
        case 2: return launch_m<2>(src, dst, plan, pitch, rule, s);
        case 4: return launch_m<4>(src, dst, plan, pitch, rule, s);
    }
    return hipErrorInvalidValue;
}

// The plan of a pass over the scratch rows of a ragged board (ceil(W / 32) words per row): rule_stream_plan's targets
RulePlan rule_stream_plan_ragged(int64_t W, int64_t H, int k, bool bounded, int64_t seg_opt) {
    return rule_stream_plan(rule_ragged_words(W) * 32, H, 1, k, bounded, seg_opt);
}

// k generations on the scratch rows of a ragged byte board: src and dst hold H rows of ceil(W / 32) words, pad bits zero
hipError_t launch_rule_stream_ragged(const uint32_t* src, uint32_t* dst, int64_t W, int64_t H, int k, bool bounded,
                                     uint32_t rule, int64_t seg_opt, hipStream_t s) {
    if (!rule_ragged_ok(W) || H < 1 || !rule_packed_ok(rule) || rule_stream_largest_k(k) != k)
        return hipErrorInvalidValue;
    const RulePlan plan = rule_stream_plan_ragged(W, H, k, bounded, seg_opt);
    if (rule_stream_grid(plan) > 0x7fffffff) return hipErrorInvalidValue;
    switch (k) {
        case 8: return launch_k_ragged<8>(src, dst, plan, W, rule, s);
        case 4: return launch_k_ragged<4>(src, dst, plan, W, rule, s);
        case 2: return launch_k_ragged<2>(src, dst, plan, W, rule, s);
        case 1: return launch_k_ragged<1>(src, dst, plan, W, rule, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace gol
