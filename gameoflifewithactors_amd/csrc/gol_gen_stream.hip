// gol_gen_stream.hip -- the multi-plane streaming pass: K generations of a Generations rule (B/S/C<n>, gol_generations.h)
// per pass over a packed board of any size, on the board's own ping-pong buffers and layout.  gol_step runs it on
// every packed board with more than two states per cell (gol_policy.cpp choose_pass).
//
// gol_rule_stream (gol_rule_step.hip) with the decay planes carried through the levels; geometry, plan and safety
// argument are that kernel's and gol_rule_plan.h's, unchanged:
//   - one wavefront per column strip of 64 blocks of M words (62 stored) and row segment (seg + 2 K rows streamed);
//   - block-edge words by DPP, a 3-row window of row sums per level rotating by static index over a trip of three
//     rows, every output row finished by rule_row<M> (rule bits as scalar branches), a scheduling barrier between levels;
//   - a row entering level l brings its P = gen_planes(nstates) decay words per alive word.  They wait in the window
//     slot beside a[l][slot] for the one step until that row is the level's centre row; then v = rule_row(...) is the
//     life-like rule's next state of the alive words and gen_decay<P>(a, v, d, masks) makes A' and D', which enter
//     level l + 1 together.  Only state-1 cells are neighbours, so the sums are the alive plane's alone.
//   - stage 0 loads 1 + P planes per row and the last level stores 1 + P.
// Bounded boards: A' is ANDed with the level's row-and-lane mask as in gol_rule_stream.  The decay needs no mask: a
// cell outside the board has A = 0 and d = 0 on entry (nothing is loaded there), so died, dying and keep are zero and
// every D' stays zero, whatever v says there.  Torus: what a halo lane's outer cells get wrong stays in those cells'
// own bits of every plane (no bit of one cell reaches another in gen_decay), and moves inward through the alive plane
// only, one cell per generation as before.
//
// nstates is a kernel argument (its C - 2 masks are scalars), P a template parameter.  Depths are 4, 2 and 1; which one
// gol_step runs per (M, P, boundary) is gen_stream_max_k (gol_gen_plan.h).
//
// gol_gen_stream_ragged below is the same pass on the whole-word scratch rows and decay planes of a ragged byte board
// (width not a multiple of 32; gol_policy.cpp use_rule_ragged).
#include "gol_internal.h"
#include "gol_bitlogic.h"
#include "gol_generations.h"
#include "gol_gen_plan.h"
#include "gol_layout.h"
#include "gol_rule.h"
#include "gol_rule_plan.h"

namespace gol {

RulePlan rule_stream_plan(int64_t W, int64_t H, int ilv, int k, bool bounded, int64_t seg_opt);  // gol_rule_step.hip

namespace {

// ---- the few device helpers of gol_rule_step.hip this kernel shares with it (that file stays as it is)
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

// rule_next_row (gol_bitlogic.h) with every rule-bit test kept a scalar branch (gol_rule_step.hip rule_row)
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

// The K windows of one wave.  Slot t % 3 of a level takes the row that enters it at step t: its row sums, its alive
// words and, beside them, its decay words.
template <int K, int M, int P, bool BOUNDED>
struct GenWindows {
    uint32_t s[K][3][M], c[K][3][M], a[K][3][M], d[K][3][P][M];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int l = 0; l < K; l++)
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int j = 0; j < M; j++) {
                    s[l][p][j] = c[l][p][j] = a[l][p][j] = 0;
#pragma unroll
                    for (int k = 0; k < P; k++) d[l][p][k][j] = 0;
                }
    }

    // One step: row (x, dx) of generation 0 enters level 0, and every level hands the row it finishes to the next; it
    // leaves as the last level's output.  yo: the row level 0 finishes at this step (bounded: level l finishes yo - l).
    template <int PH>
    __device__ __forceinline__ void step(uint32_t (&x)[M], uint32_t (&dx)[P][M], uint32_t rule, const GenMasks& g,
                                         uint32_t lanemask, int64_t yo, int64_t H) {
        constexpr int PV = (PH + 1) % 3, C = (PH + 2) % 3;
#pragma unroll
        for (int l = 0; l < K; l++) {
            const uint32_t lft = lane_left(x[M - 1]);
            const uint32_t rgt = lane_right(x[0]);
            row_sum_block<M>(x, lft, rgt, s[l][PH], c[l][PH]);
#pragma unroll
            for (int j = 0; j < M; j++) {
                a[l][PH][j] = x[j];
#pragma unroll
                for (int k = 0; k < P; k++) d[l][PH][k][j] = dx[k][j];
            }
            uint32_t v[M];
            rule_row<M>(s[l][PV], c[l][PV], s[l][C], c[l][C], s[l][PH], c[l][PH], a[l][C], rule, v);
#pragma unroll
            for (int j = 0; j < M; j++) {
                uint32_t dd[P];
#pragma unroll
                for (int k = 0; k < P; k++) dd[k] = d[l][C][k][j];
                x[j] = gen_decay<P>(a[l][C][j], v[j], dd, g);
#pragma unroll
                for (int k = 0; k < P; k++) dx[k][j] = dd[k];
            }
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

// src / dst: the alive plane; dsrc / ddst: decay plane k at + k * plane words, each plane in the board's own layout
template <int K, int M, int P, bool BOUNDED>
__global__ __launch_bounds__(64 * kRuleWavesPerBlock) void gol_gen_stream(
    const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint32_t* __restrict__ dsrc,
    uint32_t* __restrict__ ddst, RulePlan plan, int64_t pitch, int64_t plane, uint32_t rule, int nstates) {
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
    const GenMasks g = gen_masks(nstates);

    // step t's row: loaded only inside the stream, (bounded) inside the board and by lanes inside the board
    int64_t ywrap = BOUNDED ? ybase : rule_mod(ybase, H);  // the next row to load (torus: wrapped)
    auto load_row = [&](int64_t t, uint32_t (&v)[M], uint32_t (&dv)[P][M]) {
#pragma unroll
        for (int j = 0; j < M; j++) {
            v[j] = 0;
#pragma unroll
            for (int k = 0; k < P; k++) dv[k][j] = 0;
        }
        const bool row_ok = t < w.steps && (!BOUNDED || (ywrap >= 0 && ywrap < H));
        if (row_ok && lane_ld) {
            const int64_t at = ywrap * pitch + lblk * M;
            load_words<M>(src + at, v);
#pragma unroll
            for (int k = 0; k < P; k++) load_words<M>(dsrc + k * plane + at, dv[k]);
        }
        ywrap++;
        if (!BOUNDED && ywrap == H) ywrap = 0;
    };

    GenWindows<K, M, P, BOUNDED> win;
    win.clear();
    uint32_t nxt[kRuleTripRows][M], nxd[kRuleTripRows][P][M];
#pragma unroll
    for (int r = 0; r < kRuleTripRows; r++) load_row(r, nxt[r], nxd[r]);

    const int64_t nstore = w.r1 - w.r0;
#pragma nounroll
    for (int64_t T = 0; T < w.trips; T++) {
        uint32_t cur[kRuleTripRows][M], cud[kRuleTripRows][P][M];
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++)
#pragma unroll
            for (int j = 0; j < M; j++) {
                cur[r][j] = nxt[r][j];
#pragma unroll
                for (int k = 0; k < P; k++) cud[r][k][j] = nxd[r][k][j];
            }
        const int64_t t0 = T * kRuleTripRows;
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++) load_row(t0 + kRuleTripRows + r, nxt[r], nxd[r]);
        __builtin_amdgcn_sched_barrier(0);  // the prefetch stays at the top of the trip
        // the last level's output of step t is row r0 - 2 K + t
        auto finish = [&](int64_t t, uint32_t (&x)[M], uint32_t (&dx)[P][M]) {
            const int64_t o = t - 2 * K;
            if (o >= 0 && o < nstore && lane_st) {
                const int64_t at = (w.r0 + o) * pitch + sblk * M;
                store_words<M>(dst + at, x);
#pragma unroll
                for (int k = 0; k < P; k++) store_words<M>(ddst + k * plane + at, dx[k]);
            }
        };
        win.template step<0>(cur[0], cud[0], rule, g, lanemask, ybase + t0 - 1, H);
        finish(t0, cur[0], cud[0]);
        win.template step<1>(cur[1], cud[1], rule, g, lanemask, ybase + t0, H);
        finish(t0 + 1, cur[1], cud[1]);
        win.template step<2>(cur[2], cud[2], rule, g, lanemask, ybase + t0 + 1, H);
        finish(t0 + 2, cur[2], cud[2]);
    }
}

// gol_gen_stream at M = 1 on the scratch rows of a ragged byte board W cells wide: every plane H rows of plan.nblocks =
// pitch = ceil(W / 32) words, the last one partial with zero pad bits, loaded, masked and stored as in
// gol_rule_stream_ragged (gol_rule_step.hip; gol_rule_plan.h "Ragged rows"): a lane's decay words are the
// same 32 ring cells as its alive word, and the partial word's lane stores the real cells of every plane.  A kernel of
// its own beside gol_gen_stream for that kernel's reason.
template <int K, int P, bool BOUNDED>
__global__ __launch_bounds__(64 * kRuleWavesPerBlock) void gol_gen_stream_ragged(
    const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint32_t* __restrict__ dsrc,
    uint32_t* __restrict__ ddst, RulePlan plan, int64_t pitch, int64_t plane, uint32_t rule, int nstates, int64_t W) {
    constexpr int M = 1;
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kRuleWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= plan.nwaves) return;
    const RuleWave w = rule_wave(plan, wave);
    int64_t lblk, sblk;
    const bool lane_ld = rule_lane_load(plan, w, lane, &lblk) || !BOUNDED;  // (a torus lane always loads)
    const bool lane_st = rule_lane_store(plan, w, lane, &sblk);
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
    const GenMasks g = gen_masks(nstates);

    // step t's row: loaded only inside the stream, (bounded) inside the board and by lanes inside the board
    int64_t ywrap = BOUNDED ? ybase : rule_mod(ybase, H);  // the next row to load (torus: wrapped)
    auto load_row = [&](int64_t t, uint32_t (&v)[M], uint32_t (&dv)[P][M]) {
#pragma unroll
        for (int j = 0; j < M; j++) {
            v[j] = 0;
#pragma unroll
            for (int k = 0; k < P; k++) dv[k][j] = 0;
        }
        const bool row_ok = t < w.steps && (!BOUNDED || (ywrap >= 0 && ywrap < H));
        if constexpr (BOUNDED) {
            if (row_ok && lane_ld) {
                const int64_t at = ywrap * pitch + lblk;
                v[0] = src[at];
#pragma unroll
                for (int k = 0; k < P; k++) dv[k][0] = dsrc[k * plane + at];
            }
        } else if (row_ok) {
            const int64_t at = ywrap * pitch;
            if (shifted) {
                v[0] = rule_ragged_load(src + at, rw);
#pragma unroll
                for (int k = 0; k < P; k++) dv[k][0] = rule_ragged_load(dsrc + k * plane + at, rw);
            } else {
                v[0] = src[at + rw.word];
#pragma unroll
                for (int k = 0; k < P; k++) dv[k][0] = dsrc[k * plane + at + rw.word];
            }
        }
        ywrap++;
        if (!BOUNDED && ywrap == H) ywrap = 0;
    };

    GenWindows<K, M, P, BOUNDED> win;
    win.clear();
    uint32_t nxt[kRuleTripRows][M], nxd[kRuleTripRows][P][M];
#pragma unroll
    for (int r = 0; r < kRuleTripRows; r++) load_row(r, nxt[r], nxd[r]);

    const int64_t nstore = w.r1 - w.r0;
#pragma nounroll
    for (int64_t T = 0; T < w.trips; T++) {
        uint32_t cur[kRuleTripRows][M], cud[kRuleTripRows][P][M];
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++)
#pragma unroll
            for (int j = 0; j < M; j++) {
                cur[r][j] = nxt[r][j];
#pragma unroll
                for (int k = 0; k < P; k++) cud[r][k][j] = nxd[r][k][j];
            }
        const int64_t t0 = T * kRuleTripRows;
#pragma unroll
        for (int r = 0; r < kRuleTripRows; r++) load_row(t0 + kRuleTripRows + r, nxt[r], nxd[r]);
        __builtin_amdgcn_sched_barrier(0);  // the prefetch stays at the top of the trip
        // the last level's output of step t is row r0 - 2 K + t
        auto finish = [&](int64_t t, uint32_t (&x)[M], uint32_t (&dx)[P][M]) {
            const int64_t o = t - 2 * K;
            if (o >= 0 && o < nstore && lane_st) {
                const int64_t at = (w.r0 + o) * pitch + sblk;
                dst[at] = x[0] & stmask;
#pragma unroll
                for (int k = 0; k < P; k++) ddst[k * plane + at] = dx[k][0] & stmask;
            }
        };
        win.template step<0>(cur[0], cud[0], rule, g, lanemask, ybase + t0 - 1, H);
        finish(t0, cur[0], cud[0]);
        win.template step<1>(cur[1], cud[1], rule, g, lanemask, ybase + t0, H);
        finish(t0 + 1, cur[1], cud[1]);
        win.template step<2>(cur[2], cud[2], rule, g, lanemask, ybase + t0 + 1, H);
        finish(t0 + 2, cur[2], cud[2]);
    }
}

struct GenLaunch {
    const uint32_t *src, *dsrc;
    uint32_t *dst, *ddst;
    RulePlan plan;
    int64_t pitch, plane;
    uint32_t rule;
    int nstates;
    hipStream_t s;
    int64_t ragged_w = 0;
};

template <int K, int P>
hipError_t launch_kp_ragged(const GenLaunch& a) {
    const dim3 grid((unsigned)rule_stream_grid(a.plan)), block(64 * kRuleWavesPerBlock);
    if (a.plan.bounded)
        hipLaunchKernelGGL((gol_gen_stream_ragged<K, P, true>), grid, block, 0, a.s, a.src, a.dst, a.dsrc, a.ddst,
                           a.plan, a.pitch, a.plane, a.rule, a.nstates, a.ragged_w);
    else
        hipLaunchKernelGGL((gol_gen_stream_ragged<K, P, false>), grid, block, 0, a.s, a.src, a.dst, a.dsrc, a.ddst,
                           a.plan, a.pitch, a.plane, a.rule, a.nstates, a.ragged_w);
    return hipGetLastError();
}

template <int P>
hipError_t launch_p_ragged(const GenLaunch& a) {
    switch (a.plan.K) {
        case 4: return launch_kp_ragged<4, P>(a);
        case 2: return launch_kp_ragged<2, P>(a);
        case 1: return launch_kp_ragged<1, P>(a);
    }
    return hipErrorInvalidValue;
}

template <int K, int M, int P>
hipError_t launch_kmp(const GenLaunch& a) {
    const dim3 grid((unsigned)rule_stream_grid(a.plan)), block(64 * kRuleWavesPerBlock);
    if (a.plan.bounded)
        hipLaunchKernelGGL((gol_gen_stream<K, M, P, true>), grid, block, 0, a.s, a.src, a.dst, a.dsrc, a.ddst, a.plan,
                           a.pitch, a.plane, a.rule, a.nstates);
    else
        hipLaunchKernelGGL((gol_gen_stream<K, M, P, false>), grid, block, 0, a.s, a.src, a.dst, a.dsrc, a.ddst, a.plan,
                           a.pitch, a.plane, a.rule, a.nstates);
    return hipGetLastError();
}

template <int M, int P>
hipError_t launch_mp(const GenLaunch& a) {
    switch (a.plan.K) {
        case 4: return launch_kmp<4, M, P>(a);
        case 2: return launch_kmp<2, M, P>(a);
        case 1: return launch_kmp<1, M, P>(a);
    }
    return hipErrorInvalidValue;
}

template <int M>
hipError_t launch_m(const GenLaunch& a) {
    switch (gen_planes(a.nstates)) {
        case 1: return launch_mp<M, 1>(a);
        case 2: return launch_mp<M, 2>(a);
        case 3: return launch_mp<M, 3>(a);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_gen_stream(const uint32_t* src, uint32_t* dst, const uint32_t* dsrc, uint32_t* ddst, int64_t W,
                             int64_t H, int64_t pitch, int ilv, int k, bool bounded, uint32_t rule, int nstates,
                             int64_t seg_opt, hipStream_t s) {
    if ((ilv != 1 && ilv != 2 && ilv != 4) || W < 32 * ilv || W % (32 * ilv) || H < 1 || pitch < W / 32 || pitch % ilv ||
        !rule_packed_ok(rule) || (k != 4 && k != 2 && k != 1) || !gen_states_ok(nstates) || nstates < 3 || !dsrc || !ddst)
        return hipErrorInvalidValue;
    const GenLaunch a{src, dsrc, dst, ddst, rule_stream_plan(W, H, ilv, k, bounded, seg_opt), pitch, pitch * H, rule,
                      nstates, s};
    if (rule_stream_grid(a.plan) > 0x7fffffff) return hipErrorInvalidValue;
    switch (ilv) {
        case 1: return launch_m<1>(a);
        case 2: return launch_m<2>(a);
        case 4: return launch_m<4>(a);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_gen_stream_ragged(const uint32_t* src, uint32_t* dst, const uint32_t* dsrc, uint32_t* ddst, int64_t W,
                                    int64_t H, int k, bool bounded, uint32_t rule, int nstates, int64_t seg_opt,
                                    hipStream_t s) {
    if (!rule_ragged_ok(W) || H < 1 || !rule_packed_ok(rule) || (k != 4 && k != 2 && k != 1) ||
        !gen_states_ok(nstates) || nstates < 3 || !dsrc || !ddst)
        return hipErrorInvalidValue;
    const int64_t nw = rule_ragged_words(W);
    GenLaunch a{src, dsrc, dst, ddst, rule_stream_plan(nw * 32, H, 1, k, bounded, seg_opt), nw, nw * H, rule, nstates, s};
    a.ragged_w = W;
    if (rule_stream_grid(a.plan) > 0x7fffffff) return hipErrorInvalidValue;
    switch (gen_planes(nstates)) {
        case 1: return launch_p_ragged<1>(a);
        case 2: return launch_p_ragged<2>(a);
        case 3: return launch_p_ragged<3>(a);
    }
    return hipErrorInvalidValue;
}

}  // namespace gol
