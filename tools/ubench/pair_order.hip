// Microbenchmark: does the ORDER of the row-pair rule's LUTs inside a level change its issue rate at 4 waves per SIMD?
// (DESIGN.md 4.7 "dependent distance".)  One iteration is one level of the level-pipelined pass (gol_pipe.hip) on a
// trip of 4 rows of 4 words -- two row pairs, 128 v_bitop3 + 8 v_alignbit + 8 DPP moves, the pass's own LUTs
// (gol_bitlogic.h row_sum_block / pair_sum / life_next_pair) -- in one of three instruction orders, each instruction
// pinned in place by a sched_barrier:
//   emitted   the order the compiler gives the pass today: word by word, g1 -> g2 -> next of a word next to each other
//             with the following word's row sum between them (dependent distances of 1-3 for most LUTs)
//   staged4   the same LUTs stage by stage over a row's 4 words: k x4, q0 x4, q1 x4, q2 x4, g1 x4, g3 x4, g2 x4, the
//             other row's sum as filler, next x4; then the second output likewise with a DPP move as filler
//   staged8   both outputs of a pair together: g1 x8, g3 x8, g2 x8, next x8
// Prints ns per wave-level per SIMD, per rule instruction (144 a level) and per VALU instruction of the listing (the
// loop also carries 12 / 20 / 12 v_mov copies at its head: staged4 is timed with 8 more than the others), one JSON
// line per order and round; the orders alternate within a round, so the spread over rounds is the benchmark's own.
//   hipcc --offload-arch=gfx950 -O3 -I gameoflifewithactors_amd/csrc tools/ubench/pair_order.hip -o tools/ubench/pair_order
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "gol_bitlogic.h"

#define ITERS 2048
#define FENCE __builtin_amdgcn_sched_barrier(0)
// one instruction each, pinned where it is written
#define LUT(d, L, a, b, c)         \
    d = gol::lut3<L>(a, b, c);     \
    FENCE
#define ALIGN(d, hi, lo, s)           \
    d = gol::align_right(hi, lo, s);  \
    FENCE
#define ROR(d, v)                                                            \
    d = (uint32_t)__builtin_amdgcn_mov_dpp((int)(v), 0x13C, 0xf, 0xf, true); \
    FENCE
#define ROL(d, v)                                                            \
    d = (uint32_t)__builtin_amdgcn_mov_dpp((int)(v), 0x134, 0xf, 0xf, true); \
    FENCE

enum { kEmitted = 0, kStaged4 = 1, kStaged8 = 2 };
constexpr int kM = 4;

// word j's west and east words of a block row (gol_bitlogic.h row_sum_block)
#define WEST(r, j, w0) ((j) == 0 ? (w0) : (r)[(j) > 0 ? (j) - 1 : 0])
#define EAST(r, j, eN) ((j) == kM - 1 ? (eN) : (r)[(j) < kM - 1 ? (j) + 1 : 0])
#define ROWSUM_S(s, r, j, w0, eN) LUT((s)[j], 0x96, WEST(r, j, w0), (r)[j], EAST(r, j, eN))
#define ROWSUM_C(c, r, j, w0, eN) LUT((c)[j], 0xE8, WEST(r, j, w0), (r)[j], EAST(r, j, eN))

// One row pair of one level: rows a = v[r], b = v[r + 1] in, the outputs of the rows before them out (in place), the
// carried sums (sX, cX: two rows back; sY, cY, aY: the row before) moved on -- the body of gol_pipe.hip's level loop.
template <int MODE>
__device__ __forceinline__ void pair(uint32_t (&a)[kM], uint32_t (&b)[kM], uint32_t& ra, uint32_t& rb, uint32_t (&sX)[kM],
                                     uint32_t (&cX)[kM], uint32_t (&sY)[kM], uint32_t (&cY)[kM], uint32_t (&aY)[kM]) {
    uint32_t pl, w0, eN, pl2, w02, eN2, k[kM], q0[kM], q1[kM], q2[kM], sA[kM], cA[kM], sB[kM], cB[kM];
    uint32_t g1[kM], g2[kM], g3[kM], h1[kM], h2[kM], h3[kM], o0[kM], o1[kM];
    if (MODE == kEmitted) {
        ROR(pl, a[kM - 1]);
        ALIGN(w0, a[kM - 1], pl, 31);
        ROWSUM_S(sA, a, 0, w0, eN);
        ROWSUM_C(cA, a, 0, w0, eN);
#pragma unroll
        for (int j = 0; j < kM; j++) {
            LUT(k[j], 0x88, sY[j], sA[j], sA[j]);
            LUT(q0[j], 0x66, sY[j], sA[j], sA[j]);
            LUT(q1[j], 0x96, cY[j], cA[j], k[j]);
            LUT(q2[j], 0xE8, cY[j], cA[j], k[j]);
            LUT(g1[j], 0xE6, q0[j], sX[j], aY[j]);
            if (j == kM - 2) {
                ALIGN(eN, ra, a[0], 1);
            }
            if (j + 1 < kM) {
                ROWSUM_S(sA, a, j + 1, w0, eN);
            }
            LUT(g2[j], 0x5C, q2[j], aY[j], g1[j]);
            LUT(g3[j], 0x25, q1[j], q2[j], cX[j]);
            if (j + 1 < kM) {
                ROWSUM_C(cA, a, j + 1, w0, eN);
            }
            LUT(o0[j], 0x48, g1[j], g2[j], g3[j]);
        }
        ROR(pl2, b[kM - 1]);
        ALIGN(w02, b[kM - 1], pl2, 31);
        ROWSUM_S(sB, b, 0, w02, eN2);
        ROWSUM_C(cB, b, 0, w02, eN2);
        ALIGN(eN2, rb, b[0], 1);
        ROWSUM_S(sB, b, kM - 1, w02, eN2);
        ROWSUM_C(cB, b, kM - 1, w02, eN2);
#pragma unroll
        for (int j = 0; j < kM; j++) {
            LUT(h1[j], 0xE6, q0[j], sB[j], a[j]);
            if (j + 1 < kM - 1) {
                ROWSUM_S(sB, b, j + 1, w02, eN2);
            }
            LUT(h2[j], 0x5C, q2[j], a[j], h1[j]);
            LUT(h3[j], 0x25, q1[j], q2[j], cB[j]);
            if (j + 1 < kM - 1) {
                ROWSUM_C(cB, b, j + 1, w02, eN2);
            }
            LUT(o1[j], 0x48, h1[j], h2[j], h3[j]);
        }
        ROL(ra, o0[0]);
        ROL(rb, o1[0]);
    } else {
        ROR(pl, a[kM - 1]);
        ROR(pl2, b[kM - 1]);
        ALIGN(w0, a[kM - 1], pl, 31);
        ALIGN(eN, ra, a[0], 1);
#pragma unroll
        for (int j = 0; j < kM; j++) { ROWSUM_S(sA, a, j, w0, eN); }
#pragma unroll
        for (int j = 0; j < kM; j++) { ROWSUM_C(cA, a, j, w0, eN); }
        if (MODE == kStaged8) {  // both rows' sums ahead of everything else
            ALIGN(w02, b[kM - 1], pl2, 31);
            ALIGN(eN2, rb, b[0], 1);
#pragma unroll
            for (int j = 0; j < kM; j++) { ROWSUM_S(sB, b, j, w02, eN2); }
#pragma unroll
            for (int j = 0; j < kM; j++) { ROWSUM_C(cB, b, j, w02, eN2); }
        }
#pragma unroll
        for (int j = 0; j < kM; j++) { LUT(k[j], 0x88, sY[j], sA[j], sA[j]); }
#pragma unroll
        for (int j = 0; j < kM; j++) { LUT(q0[j], 0x66, sY[j], sA[j], sA[j]); }
#pragma unroll
        for (int j = 0; j < kM; j++) { LUT(q1[j], 0x96, cY[j], cA[j], k[j]); }
#pragma unroll
        for (int j = 0; j < kM; j++) { LUT(q2[j], 0xE8, cY[j], cA[j], k[j]); }
        if (MODE == kStaged4) {
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g1[j], 0xE6, q0[j], sX[j], aY[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g3[j], 0x25, q1[j], q2[j], cX[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g2[j], 0x5C, q2[j], aY[j], g1[j]); }
            ALIGN(w02, b[kM - 1], pl2, 31);  // filler: the other row's sum
            ALIGN(eN2, rb, b[0], 1);
#pragma unroll
            for (int j = 0; j < kM; j++) { ROWSUM_S(sB, b, j, w02, eN2); }
#pragma unroll
            for (int j = 0; j < kM; j++) { ROWSUM_C(cB, b, j, w02, eN2); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(o0[j], 0x48, g1[j], g2[j], g3[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h1[j], 0xE6, q0[j], sB[j], a[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h3[j], 0x25, q1[j], q2[j], cB[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h2[j], 0x5C, q2[j], a[j], h1[j]); }
            ROL(ra, o0[0]);  // filler
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(o1[j], 0x48, h1[j], h2[j], h3[j]); }
            ROL(rb, o1[0]);
        } else {
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g1[j], 0xE6, q0[j], sX[j], aY[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h1[j], 0xE6, q0[j], sB[j], a[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g3[j], 0x25, q1[j], q2[j], cX[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h3[j], 0x25, q1[j], q2[j], cB[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(g2[j], 0x5C, q2[j], aY[j], g1[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(h2[j], 0x5C, q2[j], a[j], h1[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(o0[j], 0x48, g1[j], g2[j], g3[j]); }
#pragma unroll
            for (int j = 0; j < kM; j++) { LUT(o1[j], 0x48, h1[j], h2[j], h3[j]); }
            ROL(ra, o0[0]);
            ROL(rb, o1[0]);
        }
    }
#pragma unroll
    for (int j = 0; j < kM; j++) {  // the window moves on: renames, no instruction
        sX[j] = sA[j];
        cX[j] = cA[j];
        sY[j] = sB[j];
        cY[j] = cB[j];
        aY[j] = b[j];
        a[j] = o0[j];
        b[j] = o1[j];
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_pair(uint32_t* out, uint32_t seed, int iters) {
    uint32_t v[4][kM], right[4], sX[kM], cX[kM], sY[kM], cY[kM], aY[kM];
    uint32_t x = seed * 0x9E3779B9u + threadIdx.x * 0x85EBCA6Bu + blockIdx.x;
    const auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        return x;
    };
#pragma unroll
    for (int j = 0; j < kM; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r][j] = next();
        sX[j] = next(), cX[j] = next(), sY[j] = next(), cY[j] = next(), aY[j] = next();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) right[r] = next();
    for (int it = 0; it < iters; it++) {
        FENCE;
        pair<MODE>(v[0], v[1], right[0], right[1], sX, cX, sY, cY, aY);
        pair<MODE>(v[2], v[3], right[2], right[3], sX, cX, sY, cY, aY);
    }
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < kM; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) acc ^= v[r][j] ^ right[r];
        acc ^= sX[j] ^ cX[j] ^ sY[j] ^ cY[j] ^ aY[j];
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

typedef void (*kfn)(uint32_t*, uint32_t, int);

int main() {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) {
        fprintf(stderr, "no device\n");
        return 1;
    }
    struct {
        const char* name;
        kfn f;
        int valu;  // VALU instructions per level in the listing (hipcc -S): the 144 and the loop-carried v_mov copies
    } ks[] = {{"emitted", k_pair<kEmitted>, 156}, {"staged4", k_pair<kStaged4>, 164}, {"staged8", k_pair<kStaged8>, 156}};
    constexpr int kWps = 4, kLaunches = 5, kRounds = 7, kPerIter = 2 * 72;  // 128 + 8 + 8 instructions per level
    const int blocks = cus * kWps;  // 256-thread blocks: one wave per SIMD each, 4 waves per SIMD in all
    uint32_t* out = nullptr;
    if (hipMalloc(&out, (size_t)blocks * 256 * 4) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
    for (auto& k : ks) {  // warm-up
        hipLaunchKernelGGL(k.f, dim3(blocks), dim3(256), 0, 0, out, 1u, ITERS);
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    for (int round = 0; round < kRounds; round++) {
        for (auto& k : ks) {
            (void)hipEventRecord(e0);
            for (int r = 0; r < kLaunches; r++) hipLaunchKernelGGL(k.f, dim3(blocks), dim3(256), 0, 0, out, (uint32_t)r + 2, ITERS);
            (void)hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) return 1;
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            const double levels = (double)kWps * ITERS * kLaunches;  // wave-levels per SIMD
            const double ns = ms * 1e6 / levels;
            printf("{\"order\": \"%s\", \"round\": %d, \"waves_per_simd\": %d, \"ns_per_level\": %.3f, \"ns_per_rule_instr\": %.4f, "
                   "\"valu_per_level\": %d, \"ns_per_valu_instr\": %.4f, \"cycles_at_2.4GHz\": %.3f}\n",
                   k.name, round, kWps, ns, ns / kPerIter, k.valu, ns / k.valu, ns / k.valu * 2.4);
        }
    }
    (void)hipFree(out);
    return 0;
}
