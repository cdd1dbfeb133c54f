// gol_cycles.hip -- the ensemble cycle census (gol_ensemble_cycles): for every board of a batch, after
// how many generations it enters a cycle and of what period, one wavefront per board, in one launch (gfx950).
//
// The two kernels are entry points over gol_batch_wave.h's board_census, which says what a wave does: gol_batch_cycles
// for the life-like batch (no decay plane), gol_gen_cycles for a Generations batch (1..3 decay planes).
#include "gol_batch_host.h"
#include "gol_batch_wave.h"
#include "gol_internal.h"
#include "gol_rule.h"
#include "gol_wave_dispatch.h"

namespace gol {
namespace {

// Board blockIdx.x: out[4 board ..] = transient, period, population of B_transient, generation steps run.
// PackedRule is empty (B3/S23 by life_next: the kernel as it was before rules existed), one uint32_t (any life-like
// rule by its packed masks) or one const uint32_t* (`count` packed rules, the wave's own read once as a scalar after
// the test on `board`), as in gol_batch.hip: launch_batch_cycles picks.
template <int NW, int RPL, bool BOUNDED, class... PackedRule>
__global__ __launch_bounds__(64) void gol_batch_cycles(const uint32_t* __restrict__ words, int64_t count, int W, int H,
                                                       int max_generations, int32_t* __restrict__ out,
                                                       PackedRule... packed_rule) {
    const int64_t board = blockIdx.x;
    if (board >= count) return;
    board_census<NW, RPL, BOUNDED, 0>(words, 0, board, threadIdx.x, W, H, max_generations, out, 2, packed_rule...);
}

// The same under a Generations rule of P decay planes: the rule one packed word, or a table of one per board where
// `rules` is not null.
template <int NW, int RPL, bool BOUNDED, int P>
__global__ __launch_bounds__(64) void gol_gen_cycles(const uint32_t* __restrict__ words, int64_t plane_stride,
                                                     int64_t count, int W, int H, int max_generations,
                                                     int32_t* __restrict__ out, uint32_t rule,
                                                     const uint32_t* __restrict__ rules, int nstates) {
    const int64_t board = blockIdx.x;
    if (board >= count) return;
    board_census<NW, RPL, BOUNDED, P>(words, plane_stride, board, threadIdx.x, W, H, max_generations, out, nstates, rule,
                                      rules);
}

}  // namespace

hipError_t launch_batch_cycles(const uint32_t* words, int64_t count, int64_t W, int64_t H, bool bounded,
                               int64_t max_generations, int32_t* out, uint32_t rule, bool force_table,
                               const uint32_t* rules, int nstates, hipStream_t s) {
    const int rpl = wave_resident_rpl(W, H);
    if (!rpl || !rule_packed_ok(rule) || !words || !out || count < 1 || count > kBatchCountMax ||
        max_generations < 1 || max_generations > kCycleGenerationsMax || !gen_states_ok(nstates))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)count), block(64);  // count <= 2^22
    const int w = (int)W, h = (int)H, G = (int)max_generations, nw = (int)((W + 31) / 32);
    if (nstates > 2)
        return dispatch_planes(gen_planes(nstates), [&](auto P) {
            return wave_dispatch(
                [&](auto NW, auto RPL, auto B) {
                    hipLaunchKernelGGL((gol_gen_cycles<NW, RPL, B, P>), grid, block, 0, s, words, count * H * nw, count,
                                       w, h, G, out, rule, rules, nstates);
                    return hipGetLastError();
                },
                nw, rpl, bounded);
        });
    const auto launch = [&](auto NW, auto RPL, auto B) {
        switch (rule_family(rule, force_table, rules)) {
            case RuleFamily::Life:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B>), grid, block, 0, s, words, count, w, h, G, out);
                break;
            case RuleFamily::Table:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B, uint32_t>), grid, block, 0, s, words, count, w, h, G,
                                   out, rule);
                break;
            case RuleFamily::PerBoard:
                hipLaunchKernelGGL((gol_batch_cycles<NW, RPL, B, const uint32_t*>), grid, block, 0, s, words, count, w,
                                   h, G, out, rules);
                break;
        }
        return hipGetLastError();
    };
    return wave_dispatch(launch, nw, rpl, bounded);
}

}  // namespace gol
