// gol_wave_shape.h -- which boards fit one wavefront's registers, and with how many rows per lane: the one statement of
// the geometry of gol_wave.hip, gol_batch.hip and gol_cycles.hip (gol_wave_body.h).  No HIP here: the pass choice
// (gol_policy.cpp) and the batch handle (gol_batch_host.h) use it, and tests/cpp/test_batch_host.cpp compiles it alone.
#pragma once
#include <stdint.h>

namespace gol {

// Rows per lane for a W x H board: the fewest (1..4) that divide H with at most 64 lanes, for W in 3..128; 0 = the
// board does not fit.
inline int wave_resident_rpl(int64_t W, int64_t H) {
    if (W < 3 || W > 128 || H < 3) return 0;
    for (int r = 1; r <= 4; r++)
        if (H % r == 0 && H / r <= 64) return r;
    return 0;
}

// Rows per lane under the rule family of the single-wave pass (any rule but B3/S23, or "rule_table"):
// wave_resident_rpl where it takes the board, else the fewest (2..4) that hold H rows in at most 64 lanes with the last
// lane partly filled, or 0.  Every board up to 128 x 256.
inline int wave_rule_rpl(int64_t W, int64_t H) {
    if (const int r = wave_resident_rpl(W, H)) return r;
    if (W < 3 || W > 128 || H < 3 || H > 256) return 0;  // (H > 256: more than 64 lanes of 4, and no overflow below)
    for (int r = 2; r <= 4; r++)
        if ((H + r - 1) / r <= 64) return r;
    return 0;
}

}  // namespace gol
