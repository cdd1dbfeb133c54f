// gol_bitlogic.h -- bit-sliced B3/S23 for 32 cells per 32-bit word (host + gfx950 device), and at the end of the file
// the same for any life-like rule given as two masks (rule_next_row; the batch handle's rules).
//
// Replaces, for 32 cells at once, the per-cell neighbour gather and rule of the reference actor:
//   GameOfLife/GameOfLife/GameOfLifeLogic.fs:56-63  (Akka: GameOfLifeAkka/GameofLife.fs:105-112)
//   a = #alive among 8 neighbours;  a > 3 || a < 2 -> dead;  a = 3 -> alive;  otherwise keep isAlive.
//
// Packing: bit b of word w in row y is cell (x = 32*w + b, y); LSB = smallest x (matches the
// reference's pixels[x + y*size] orientation, GameOfLifeUI.fs:27).
//
// Arithmetic (13 VALU ops per word per generation on gfx950, 2 of them DPP moves done by the caller):
//   row sum   W + C + E of one row as a 2-bit number (s, c): 2 x v_alignbit_b32 + 2 x v_bitop3_b32
//             (xor3 = LUT 0x96, majority = LUT 0xE8)
//   vertical  t = sP + sC + sN + 2 (cP + cC + cN) is the 9-cell sum including the centre; the rule is
//             next = (t == 3) | (alive & t == 4).  A = xor3(s), B = maj3(s), X = xor3(c), Y = maj3(c)
//             then a 3-LUT tree found by exhaustive search (tests/cpp/test_bitlogic.cpp re-checks all 2^9
//             neighbourhoods):  o1 = L(A, Y, alive; 0x27), o2 = L(B, X, Y; 0x19), next = L(o1, o2, A; 0x24).
//   row pairs the pipelined pass (gol_pipe.hip) takes its rows two at a time and shares the vertical sum of the two rows
//             both outputs hold (pair_sum / life_next_pair below): 2 + 2 + 4 = 8 LUT ops per word and generation
//             instead of 2 + 4 + 3 = 9, i.e. 12 VALU ops with the caller's shifts and moves at one word per block.
//
// LUT convention used in this file: lut3(a, b, c, L) = bit (a | b<<1 | c<<2) of L.  gfx950's
// v_bitop3_b32 indexes its immediate with (S0<<2 | S1<<1 | S2), so a -> S2 and c -> S0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GOL_HD __host__ __device__ __forceinline__
#else
#define GOL_HD static inline
#endif

namespace gol {

template <unsigned L>
GOL_HD uint32_t lut3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(c, b, a, L);
#else
    uint32_t r = 0;
    for (unsigned i = 0; i < 8; i++)
        if ((L >> i) & 1u) r |= ((i & 1u) ? a : ~a) & ((i & 2u) ? b : ~b) & ((i & 4u) ? c : ~c);
    return r;
#endif
}
GOL_HD uint32_t align_right(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
#endif
}

// Horizontal 3-sum of one row around each of 32 cells: (prev word, this word, next word) -> (s, c).
GOL_HD void row_sum(uint32_t prev, uint32_t cur, uint32_t next, uint32_t& s, uint32_t& c) {
    const uint32_t w = align_right(cur, prev, 31);  // west neighbour of every cell
    const uint32_t e = align_right(next, cur, 1);   // east neighbour of every cell
    s = lut3<0x96>(w, cur, e);
    c = lut3<0xE8>(w, cur, e);
}

// Horizontal 3-sums of one block of M interleaved words (gol_layout.h: word j bit b = cell j + M*b).
// West of word j is word j-1 at the same bit, except word 0 whose west is word M-1 one bit lower (the
// bit below bit 0 comes from the previous block's word M-1, `prev_last`); symmetrically for east.
// So a block costs 2 funnel shifts whatever M is (M = 1 reduces to row_sum above).
template <int M>
GOL_HD void row_sum_block(const uint32_t (&r)[M], uint32_t prev_last, uint32_t next_first, uint32_t (&s)[M],
                          uint32_t (&c)[M]) {
    const uint32_t w0 = align_right(r[M - 1], prev_last, 31);
    const uint32_t eN = align_right(next_first, r[0], 1);
#pragma unroll
    for (int j = 0; j < M; j++) {
        const uint32_t w = j == 0 ? w0 : r[j - 1];
        const uint32_t e = j == M - 1 ? eN : r[j + 1];
        s[j] = lut3<0x96>(w, r[j], e);
        c[j] = lut3<0xE8>(w, r[j], e);
    }
}

// Next state of 32 cells from the three row sums (previous, centre, next row) and the centre word.
GOL_HD uint32_t life_next(uint32_t sP, uint32_t cP, uint32_t sC, uint32_t cC, uint32_t sN, uint32_t cN,
                          uint32_t alive) {
    const uint32_t A = lut3<0x96>(sP, sC, sN);
    const uint32_t B = lut3<0xE8>(sP, sC, sN);
    const uint32_t X = lut3<0x96>(cP, cC, cN);
    const uint32_t Y = lut3<0xE8>(cP, cC, cN);
    const uint32_t o1 = lut3<0x27>(A, Y, alive);
    const uint32_t o2 = lut3<0x19>(B, X, Y);
    return lut3<0x24>(o1, o2, A);
}

// ---- two output rows at once: 8 LUT ops per word and generation (the pipelined pass, gol_pipe.hip).
//
// Rows n and n + 1 entering a level give the outputs of rows n - 1 and n, and both 9-cell totals hold the same two
// middle rows:  t(n - 1) = row(n - 2) + [row(n - 1) + row(n)],  t(n) = [row(n - 1) + row(n)] + row(n + 1).
// pair_sum adds the shared pair once, as a 3-bit number q = q0 + 2 q1 + 4 q2 = (s1 + 2 c1) + (s2 + 2 c2) in 0..6
// (4 ops per word for two output rows); life_next_pair finishes one output from q, the remaining row's sum (s, c) and
// the output's own centre word (4 ops), so 2 (row sum) + 2 + 4 = 8 against life_next's 2 + 7.
//   t = q + s + 2 c  (0..9);  next = (t == 3) | (alive & t == 4), as life_next.
//   g1 = L(q0, s, alive; 0xE6) = alive ? q0 | s : q0 ^ s     -- t's low bit for a dead cell, "t0 or a carry" for a live
//   g2 = L(q2, alive, g1; 0x5C),  g3 = L(q1, q2, c; 0x25),  next = L(g1, g2, g3; 0x48)
// a 4-LUT circuit found by exhaustive search over the reachable inputs.  It relies on two don't-cares that hold by
// construction: q != 7 (two 2-bit row sums of at most 3 each), and alive => q >= 1 (the centre word is one of the pair's
// two rows, and a live centre is counted in its own row's sum).  Outside them the circuit is NOT life_next: `alive` must
// be the centre word of a row whose sum went into q.  tests/cpp/test_bitlogic_pair.cpp checks both outputs against
// life_next over all 2^12 fillings of a 4 x 3 neighbourhood and over random words on a small interleaved torus.
GOL_HD void pair_sum(uint32_t s1, uint32_t c1, uint32_t s2, uint32_t c2, uint32_t& q0, uint32_t& q1, uint32_t& q2) {
    // Two-input ops written as LUTs that ignore their third input (0x88 = a & b, 0x66 = a ^ b): the compiler emits
    // `s1 & s2` and `s1 ^ s2` as 4-byte v_and_b32 / v_xor_b32, and a 4-byte instruction inside one of the pipelined
    // pass's levels flips the address parity of every 8-byte instruction after it (gol_pipe.hip level_align)
    const uint32_t k = lut3<0x88>(s1, s2, s2);
    q0 = lut3<0x66>(s1, s2, s2);
    q1 = lut3<0x96>(c1, c2, k);
    q2 = lut3<0xE8>(c1, c2, k);
}
GOL_HD uint32_t life_next_pair(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t s, uint32_t c, uint32_t alive) {
    const uint32_t g1 = lut3<0xE6>(q0, s, alive);
    const uint32_t g2 = lut3<0x5C>(q2, alive, g1);
    const uint32_t g3 = lut3<0x25>(q1, q2, c);
    return lut3<0x48>(g1, g2, g3);
}

// ---- the same circuit on a block of M words, one LUT of the circuit for all M words at a time (gol_pipe.hip).
//
// Word by word, g1 -> g2 -> next of a word follow each other at distances of 1-3 instructions, and at 4 waves per SIMD
// a v_bitop3 that close behind its producer issues 4-12 % slower than one 8 or more behind (DESIGN.md 4.7 "dependent
// distance").  Stage by stage over M = 4 words, with the caller's filler between g2 and next, every LUT is 4 or more
// behind its producer and most are 8 or more.  The stages are the LUTs of pair_sum / life_next_pair, same immediates.
// stage_end() closes a stage: on the device an empty asm reads the stage's results (no instruction, and no register
// written: an asm that defined them would look like a VALU write to the hazard recognizer, which then pads the level
// with 4-byte s_nops), so the stage's LUTs stay ahead of it whatever the optimizer would rather do, and a sched_barrier
// keeps the instruction scheduler from interleaving the stages again; on the host it is nothing.
// tests/cpp/test_bitlogic_pair_block.cpp checks the block forms against life_next_pair and life_next.
GOL_HD void stage_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0x4 | 0x10 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200);  // all but VALU may cross
#endif
}
GOL_HD void stage_end(const uint32_t& x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : : "v"(x));
#else
    (void)x;
#endif
    stage_fence();
}
template <int M>
GOL_HD void stage_end(const uint32_t (&x)[M]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int j = 0; j < M; j++) asm volatile("" : : "v"(x[j]));
#else
    (void)x;
#endif
    stage_fence();
}
// row_sum_block from the two funnel shifts the caller made ahead of it (w0 = align_right(r[M - 1], prev_last, 31),
// eN = align_right(next_first, r[0], 1)): s of the words between, of word M - 1, of word 0, one by one; then c x M
template <int M>
GOL_HD void row_sum_block_staged(const uint32_t (&r)[M], uint32_t w0, uint32_t eN, uint32_t (&s)[M], uint32_t (&c)[M]) {
#pragma unroll
    for (int i = 0; i < M; i++) {
        const int j = i == M - 1 ? 0 : i + 1;  // 1 .. M - 1, 0
        s[j] = lut3<0x96>(j == 0 ? w0 : r[j > 0 ? j - 1 : 0], r[j], j == M - 1 ? eN : r[j < M - 1 ? j + 1 : 0]);
        stage_end(s[j]);
    }
#pragma unroll
    for (int j = 0; j < M; j++)
        c[j] = lut3<0xE8>(j == 0 ? w0 : r[j > 0 ? j - 1 : 0], r[j], j == M - 1 ? eN : r[j < M - 1 ? j + 1 : 0]);
    stage_end(c);
}
// pair_sum: k x M, q0 x M, q1 x M, q2 x M
template <int M>
GOL_HD void pair_sum_block(const uint32_t (&s1)[M], const uint32_t (&c1)[M], const uint32_t (&s2)[M],
                           const uint32_t (&c2)[M], uint32_t (&q0)[M], uint32_t (&q1)[M], uint32_t (&q2)[M]) {
    uint32_t k[M];
#pragma unroll
    for (int j = 0; j < M; j++) k[j] = lut3<0x88>(s1[j], s2[j], s2[j]);
    stage_end(k);
#pragma unroll
    for (int j = 0; j < M; j++) q0[j] = lut3<0x66>(s1[j], s2[j], s2[j]);
    stage_end(q0);
#pragma unroll
    for (int j = 0; j < M; j++) q1[j] = lut3<0x96>(c1[j], c2[j], k[j]);
    stage_end(q1);
#pragma unroll
    for (int j = 0; j < M; j++) q2[j] = lut3<0xE8>(c1[j], c2[j], k[j]);
    stage_end(q2);
}
// life_next_pair in three steps: g1 x M and g3 x M; g2 x M; (the caller's filler;) next x M
template <int M>
GOL_HD void pair_g13_block(const uint32_t (&q0)[M], const uint32_t (&q1)[M], const uint32_t (&q2)[M],
                           const uint32_t (&s)[M], const uint32_t (&c)[M], const uint32_t (&alive)[M], uint32_t (&g1)[M],
                           uint32_t (&g3)[M]) {
#pragma unroll
    for (int j = 0; j < M; j++) g1[j] = lut3<0xE6>(q0[j], s[j], alive[j]);
    stage_end(g1);
#pragma unroll
    for (int j = 0; j < M; j++) g3[j] = lut3<0x25>(q1[j], q2[j], c[j]);
    stage_end(g3);
}
template <int M>
GOL_HD void pair_g2_block(const uint32_t (&q2)[M], const uint32_t (&alive)[M], const uint32_t (&g1)[M], uint32_t (&g2)[M]) {
#pragma unroll
    for (int j = 0; j < M; j++) g2[j] = lut3<0x5C>(q2[j], alive[j], g1[j]);
    stage_end(g2);
}
template <int M>
GOL_HD void pair_next_block(const uint32_t (&g1)[M], const uint32_t (&g2)[M], const uint32_t (&g3)[M], uint32_t (&out)[M]) {
#pragma unroll
    for (int j = 0; j < M; j++) out[j] = lut3<0x48>(g1[j], g2[j], g3[j]);
    stage_end(out);
}

// ---- any life-like rule (gol_rule.h: birth | survive << 9, uniform over a launch) on N words of one row at a time.
//
// t = A + 2 (B + X) + 4 Y is the 9-cell total, 0..9, as four bit planes: t0 = A, t1 = B ^ X, t2 = Y ^ (B & X),
// t3 = Y & B & X.  A dead cell with n neighbours has t = n, a live one t = n + 1, so
//   next = OR over set birth bits n of (t == n & ~alive)  |  OR over set survive bits n of (t == n + 1 & alive).
// For t <= 7 a term is a minterm of (t0, t1, t2) -- one LUT with a compile-time immediate -- under a qualifier word
// (~t3 & ~alive or ~t3 & alive, made once), ORed in by one a | (b & c).  t >= 8 leaves t1 = t2 = 0, so birth 8 is
// t3 & ~t0 & ~alive, survive 7 is t3 & ~t0 & alive and survive 8 is t3 & t0 & alive: one LUT and one OR each.  Every
// term sits under a test of its rule bit -- a scalar branch on the device, taken once for the N words -- so a clear bit
// costs no vector instruction: 9 fixed and 2 per set bit, per word.
//
// SURVIVE only names the planes in the other order (t2, t1, t0: the minterm of V is then bit rev3(V) of the LUT).  Birth
// n + 1 and survive n test the same t, and given one spelling of that minterm the compiler computes it ahead of both
// branches, for all seven t and whatever the rule: 7 instructions per word that a rule of three or four digits never
// needs.
template <unsigned V, bool SURVIVE, int N>
GOL_HD void rule_term(uint32_t (&acc)[N], const uint32_t (&t0)[N], const uint32_t (&t1)[N], const uint32_t (&t2)[N],
                      const uint32_t (&q)[N]) {
    constexpr unsigned R = (V & 1u) << 2 | (V & 2u) | (V & 4u) >> 2;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint32_t m = SURVIVE ? lut3<(1u << R)>(t2[j], t1[j], t0[j]) : lut3<(1u << V)>(t0[j], t1[j], t2[j]);
        acc[j] = lut3<0xEA>(acc[j], m, q[j]);
    }
}
template <unsigned L, int N>
GOL_HD void rule_term_high(uint32_t (&acc)[N], const uint32_t (&t3)[N], const uint32_t (&t0)[N],
                           const uint32_t (&alive)[N]) {
#pragma unroll
    for (int j = 0; j < N; j++) acc[j] |= lut3<L>(t3[j], t0[j], alive[j]);
}

template <int N>
GOL_HD void rule_next_row(const uint32_t (&sP)[N], const uint32_t (&cP)[N], const uint32_t (&sC)[N],
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
        t2[j] = lut3<0x78>(B, X, Y);  // (a & b) ^ c
        t3[j] = lut3<0x80>(B, X, Y);  // a & b & c
        qd[j] = ~(t3[j] | alive[j]);
        qa[j] = alive[j] & ~t3[j];
        acc[j] = 0;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // The rule stays one scalar register tested here bit by bit (s_bitcmp1_b32, s_cbranch_scc): hoisted out of the
    // generation loop the 18 tests become 18 lane masks in register pairs, re-tested by vector compares.
    asm volatile("" : "+s"(rule));
#endif
    if (rule >> 0 & 1) rule_term<0, false>(acc, t0, t1, t2, qd);  // birth n: t == n, dead
    if (rule >> 1 & 1) rule_term<1, false>(acc, t0, t1, t2, qd);
    if (rule >> 2 & 1) rule_term<2, false>(acc, t0, t1, t2, qd);
    if (rule >> 3 & 1) rule_term<3, false>(acc, t0, t1, t2, qd);
    if (rule >> 4 & 1) rule_term<4, false>(acc, t0, t1, t2, qd);
    if (rule >> 5 & 1) rule_term<5, false>(acc, t0, t1, t2, qd);
    if (rule >> 6 & 1) rule_term<6, false>(acc, t0, t1, t2, qd);
    if (rule >> 7 & 1) rule_term<7, false>(acc, t0, t1, t2, qd);
    if (rule >> 8 & 1) rule_term_high<0x02>(acc, t3, t0, alive);  // t == 8, dead: a & ~b & ~c
    if (rule >> 9 & 1) rule_term<1, true>(acc, t0, t1, t2, qa);  // survive n: t == n + 1, alive
    if (rule >> 10 & 1) rule_term<2, true>(acc, t0, t1, t2, qa);
    if (rule >> 11 & 1) rule_term<3, true>(acc, t0, t1, t2, qa);
    if (rule >> 12 & 1) rule_term<4, true>(acc, t0, t1, t2, qa);
    if (rule >> 13 & 1) rule_term<5, true>(acc, t0, t1, t2, qa);
    if (rule >> 14 & 1) rule_term<6, true>(acc, t0, t1, t2, qa);
    if (rule >> 15 & 1) rule_term<7, true>(acc, t0, t1, t2, qa);
    if (rule >> 16 & 1) rule_term_high<0x20>(acc, t3, t0, alive);  // t == 8, alive: a & ~b & c
    if (rule >> 17 & 1) rule_term_high<0x80>(acc, t3, t0, alive);  // t == 9, alive: a & b & c
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = acc[j];
}

// The same seven inputs as life_next, 32 cells.
GOL_HD uint32_t rule_next(uint32_t sP, uint32_t cP, uint32_t sC, uint32_t cC, uint32_t sN, uint32_t cN, uint32_t alive,
                          uint32_t rule) {
    const uint32_t a[7][1] = {{sP}, {cP}, {sC}, {cC}, {sN}, {cN}, {alive}};
    uint32_t out[1];
    rule_next_row<1>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], rule, out);
    return out[0];
}

}  // namespace gol
