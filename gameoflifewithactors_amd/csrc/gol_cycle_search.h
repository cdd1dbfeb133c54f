// gol_cycle_search.h -- the control flow of the ensemble cycle census (gol_ensemble_cycles): transient
// and period of a deterministic sequence B_0, B_1 = step(B_0), ..., within a budget of G generations.  No HIP here: the
// kernel (gol_cycles.hip) instantiates it on a board held in one wave's registers, tests/cpp/test_cycle_search.cpp on a
// toy sequence under the sanitizers, so the control flow the GPU runs is the one checked exhaustively on the CPU.
//
// Definition.  t* = the smallest t >= 1 with B_t = B_s for some s < t; transient mu = s, period lambda = t* - mu.
// Resolved exactly when t* = mu + lambda <= G; otherwise (-1, 0), whatever the search happened to see beyond G.
//
// Phase 1 (Brent) finds lambda.  A saved state T, first B_0, and a window p = 1: step the hare; hare == T after `since`
// steps means lambda = since; after p steps without a hit T <- hare, p <- 2 p.  T is taken at generations 2^k - 1 and
// the hit comes at generation 2^k - 1 + lambda for the smallest 2^k >= max(mu + 1, lambda), which is below
// 2 max(mu + 1, lambda) - 1 + lambda < 3 t*.  So a hare stopped at generation 3 G loses no sequence with t* <= G, and
// lambda is exact: T lies on the cycle, and the first return to a state on the cycle is after exactly lambda steps.
// Phase 2 finds mu.  A <- B_0, B <- B_lambda (lambda steps), both stepped in lockstep until A == B: A = B_mu.  It gives
// up as soon as mu + lambda would exceed G.
//
// Budgets.  Phase 1 runs at most 3 G steps, phase 2 at most lambda + 2 (G - lambda) < 2 G: `steps` <= 5 G, inside the
// documented 6 G.  Every loop bound below is a counter derived from G alone (`limit`, and lambda only after it has been
// found <= G): no sequence, and no fault in `equal`, can make a loop run on.
//
// State type S: copyable and assignable, `void step()`, `bool equal(const S&) const`.  `load()` returns B_0; the search
// calls it up to three times, so the kernel re-reads its board from memory where a third copy would cost registers.
// On the GPU every lane of the wave runs this code: `equal` must return the same value in every lane.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GOL_CYCLE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GOL_CYCLE_HD inline
#endif

namespace gol {

constexpr int32_t kCycleGenerationsMax = (int32_t)1 << 20;  // G of one call: 6 G fits 32 bits with room to spare

struct CycleResult {
    int32_t transient;  // mu, or -1 when unresolved
    int32_t period;     // lambda, or 0 when unresolved
    int32_t steps;      // calls of S::step(): cost accounting, <= 6 G
};

// `at_hit(A)` is called once, with A = B_mu, when (and only when) the sequence is resolved.
template <class S, class Load, class AtHit>
GOL_CYCLE_HD CycleResult cycle_search(Load&& load, int32_t G, AtHit&& at_hit) {
    CycleResult r = {-1, 0, 0};
    if (G < 1 || G > kCycleGenerationsMax) return r;
    int32_t lambda = 0;
    {
        S T = load();
        S hare = T;
        const int32_t limit = 3 * G;  // the hare's last generation
        int32_t p = 1, since = 0;
        for (int32_t gen = 0; gen < limit; gen++) {
            hare.step();
            r.steps++;
            since++;
            if (hare.equal(T)) {
                lambda = since;
                break;
            }
            if (since == p) {
                T = hare;
                p *= 2;  // p <= 2^k with 2^k - 1 <= 3 G < 2^22
                since = 0;
            }
        }
    }
    if (lambda < 1 || lambda > G) return r;  // no hit by 3 G, or t* >= lambda > G
    S A = load();
    S B = A;
    for (int32_t i = 0; i < lambda; i++) {  // lambda <= G
        B.step();
        r.steps++;
    }
    const int32_t last = G - lambda;  // the largest mu with mu + lambda <= G
    for (int32_t mu = 0; mu <= last; mu++) {
        if (A.equal(B)) {
            r.transient = mu;
            r.period = lambda;
            at_hit(A);
            return r;
        }
        if (mu == last) break;  // the next mu is beyond the budget: not stepped for
        A.step();
        B.step();
        r.steps += 2;
    }
    return r;
}

}  // namespace gol
