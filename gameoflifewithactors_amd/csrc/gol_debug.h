/*
 * gol_debug.h -- test and A/B knobs of libgol_hip.so (internal: not part of the drop-in boundary include/gol/gol.h).
 *
 * These change how a pass is launched or let a test drive a rare state early; unlike gol.h's gol_set_option names,
 * some of them are not results-neutral by themselves (a spin limit of one poll makes a hand-off time out and the
 * board invalid), so the F# drop-in does not bind them.  The tests and the A/B tools reach them through ctypes.
 *   "coop_epoch" 0..65535       the tag epoch of the last persistent launch (the next runs at value + 1); setting it
 *                               clears the hand-off granules, so no stale granule can match a later launch's tag
 *   "coop_spin_limit" 0 | n     polls before a hand-off wait gives up and marks the board invalid (0: ~2 s)
 *   "coop_r" 1..8               cooperative pass: rows per wave at least (A/B)
 *   "resident_threads" 1024 | 256  LDS-resident pass workgroup size (A/B)
 *   "coop_launch" 0 | 1         persistent passes by hipLaunchKernel after a residency check (0), or by
 *                               hipLaunchCooperativeKernel (1; DESIGN.md 6 "Exit under rocprofv3")
 *   "lanes_launches"            (read-only) launches of the rows-on-lanes pass on this board
 *   "last_pass"                 (read-only) the pass the last gol_step / gol_step_timed call took, as gol::Pass
 *                               (gol_board.h): 0 none yet, 1 single-wave, 2 rows-on-lanes, 3 cooperative, 4 cooperative on
 *                               a ragged board's scratch rows, 5 block (ring) rows, 6 ragged streaming, 7 LDS-resident,
 *                               8 byte step, 9 streaming, 10 multi-part, 11 rule-generic streaming,
 *                               12 multi-plane streaming (Generations), 13 / 14 those two on a ragged board's scratch rows
 *   "rule_table" 0 | 1          1: a B3/S23 board runs the passes of the rule family too (single-wave with the rule
 *                               table, rule-generic streaming, byte step under the rule), as any other rule always
 *                               does.  Results are identical: the knob is what lets the rule arithmetic be checked
 *                               against the B3/S23 passes and the committed goldens, and timed against them
 *                               (DESIGN.md 4.12).  Multi-part boards refuse 1 (GOL_ERR_UNSUPPORTED)
 *   "rule_k" 0 | 1 | 2 | 4 | 8  the deepest pass of the rule-generic streaming pass (0: by layout; A/B)
 *   "rule_seg_rows" 0 | n       rows per wave segment of the rule-generic streaming pass (0: planned): small test
 *                               boards get several segments
 *                               Both apply to the multi-plane streaming pass of a Generations board too:
 *                               "rule_k" 4, 2, 1 force its depth, 8 is refused there (GOL_ERR_INVALID); and to both
 *                               passes on a ragged board's scratch rows
 * Unknown names return GOL_ERR_INVALID.
 */
#ifndef GOL_DEBUG_H
#define GOL_DEBUG_H

#include <stdint.h>

#include "gol/gol.h"

#ifdef __cplusplus
extern "C" {
#endif

int gol_debug_set_option(gol_board* b, const char* name, int64_t value);
int gol_debug_get_option(gol_board* b, const char* name, int64_t* value);
/* The names above, comma-separated (the library's own list: _lib.DEBUG_OPTIONS is tested against it). */
const char* gol_debug_option_names(void);
/* Level-pipelined pass (gol_pipe.hip): its plan for a strip pass with `wgs` resident workgroups (0: the device's) and
 * the violations a host walk of it finds -- plan[15] = nstrips, rem, rq, rp, ngroups, grows, pk_lo, pk_hi, npk, nrem,
 * P, split1, split2, grid, violations -- and the library's own error word of its strip passes (read and cleared). */
int gol_debug_pipe_plan(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t wgs, int64_t* plan,
                        int64_t n);
int gol_debug_pipe_errors(int* out);
/* Batch handle (gol_batch.hip): boards (wavefronts) per workgroup of its step launches, 1 (the default) or 4 -- the
 * workgroup-shape A/B of DESIGN.md 4.9.  Results are identical. */
int gol_debug_batch_group_waves(gol_batch* b, int waves);
/* Batch handle: with force = 1 a B3/S23 batch runs the rule-table kernels too (any other rule always does; 0, the
 * default, leaves B3/S23 on the life_next kernels).  Results are identical: the knob is what lets the table arithmetic
 * be checked against life_next on the same boards, and timed against it. */
int gol_debug_batch_rule_table(gol_batch* b, int force);
/* Device time of the handle's last successful gol_ensemble_cycles launch, between two HIP events on its stream around
 * the kernel alone (the copy of the results is outside them); GOL_ERR_INVALID before the first such call. */
int gol_debug_ensemble_cycles_us(gol_batch* b, double* elapsed_us);

#ifdef __cplusplus
}
#endif
#endif /* GOL_DEBUG_H */
