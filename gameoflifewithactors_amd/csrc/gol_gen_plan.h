// gol_gen_plan.h -- the depth table of the multi-plane streaming pass (gol_gen_stream.hip).  Host-only,
// no HIP: gol_passes.cpp asks it, tests/cpp/test_gen_board.cpp walks it, and tests/test_cpu_gen_stream_envelope.py holds
// it against the register counts of the compiled kernels.
#pragma once

namespace gol {

constexpr int kGenStreamDepths[] = {4, 2, 1};  // the depths gol_gen_stream is instantiated at
constexpr int kGenStreamMaxVgprs = 256;        // two waves per SIMD of 512 registers

// The deepest pass gol_step runs on a board of layout ilv (words per block: 1, 2, 4) with `planes` decay planes
// (1..3): the deepest of 4, 2, 1 whose kernel has no scratch and at most kGenStreamMaxVgprs registers, that is at
// least two waves per SIMD.  A condition, not a measurement: the pass is latency-bound (one dependent chain per wave),
// and the rule stream's K = 8 at one wave per SIMD lost 2x to K = 4.  The registers of every kernel
// are in DESIGN.md 4.15; 0 for a layout or plane count the pass does not have.
constexpr int gen_stream_max_k(int ilv, int planes, bool bounded) {
    if ((ilv != 1 && ilv != 2 && ilv != 4) || planes < 1 || planes > 3) return 0;
    if (ilv < 4) return 4;
    (void)bounded;
    return planes == 1 ? 4 : 2;
}

// The depth of the next pass with `left` generations to go under a cap of 4, 2 or 1
constexpr int gen_stream_largest_k(long long left, int cap) {
    return left >= 4 && cap >= 4 ? 4 : (left >= 2 && cap >= 2 ? 2 : (left >= 1 ? 1 : 0));
}

}  // namespace gol
