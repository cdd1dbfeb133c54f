// gol_stream_plan.cpp -- host planner of the streaming pass (gol_step.hip): the depth a step may use, the strip and
// segment decomposition of a pass (plan_stream: one balanced round of resident waves, the SIMD-group splits, the seam
// geometry's remainder units) and the arguments handed on to the level-pipelined pass.  Plain integer arithmetic: it
// shares the strip constants with the kernel through gol_layout.h and asks gol_step.hip for a variant's workgroup
// size and residency (stream_wpb, resident_units), so a split constant can change without recompiling the kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_layout.h"
#include "gol_internal.h"

namespace gol {

int stream_max_k(int ilv) { return ilv == 1 ? 32 : (ilv == 2 ? 16 : 32); }

int stream_largest_k(int64_t n, int cap, int ilv, int64_t words, bool bounded) {
    static const int ks[] = {32, 24, 16, 12, 8, 6, 4, 2, 1};
    for (int k : ks) {
        if (k > cap || k > n || !stream_supported(k, ilv)) continue;
        // the level-pipelined depths (16 / 32 at ilv 4) only where that pass runs (torus rows of a full strip)
        if (ilv == 4 && pipe_supported(k) && !pipe_applies(words, ilv, k, bounded, 0)) continue;
        return k;
    }
    return 1;
}

int64_t stream_strips(int64_t words, int ilv, int k, bool bounded, int rag_bits) {
    const int64_t nblocks = words / ilv;
    if (rag_bits && !bounded) return (nblocks + kInterior - 1) / kInterior;  // ragged torus rows: see plan_stream
    if (k == 1) return (nblocks + kWave - 1) / kWave;  // K = 1: halo-free strips
    // bounded edge-fill strips (StreamWave::edge_fill): strip 0 stores blocks [0, 63), strip s stores
    // [62 s + 1, 62 s + 63), the last ends at the board's last block
    if (bounded && nblocks >= kWave) return (nblocks - 1 + kInterior - 1) / kInterior;
    // halo-lane strips (torus; bounded NARROW = 1: narrow rows): strip s stores blocks [62 s, 62 s + 62)
    return (nblocks + kInterior - 1) / kInterior;
}

// Pair split (1/65536 units): the share of a pair segment given to the older of the two waves that
// share a SIMD.  VALU issue favours the older wave (MI355X_MICROARCH.md "Two waves per SIMD"), so with
// equal segments it finishes early and leaves the younger alone at the single-wave issue rate
// (tools/tail.py: 65536^2, K = 16 -- waves 0-3 of every workgroup busy 489 us, waves 4-7 747 us).
// A board's "split" option (gol_set_option) overrides it for experiments.
int stream_pair_split(int k, int ilv, bool bounded, bool wrap, bool single) {
    if (kWavesPerBlock < 8) return 0;
    // Round 5, with the middle wave's share set apart (stream_split2), at the bench window (generation 300+), 4
    // interleaved rounds (profiles/r5/split2_confirm_g.jsonl, us per pass, mean): single-board torus (12, 2) 0.66 / 0.76
    // 442.5 against 0.70 / geometric 445.8; bounded (12, 2) 0.60 / 0.72 431.0 against 0.64 / geometric 436.0.  The
    // per-role tails of a stamped build (profiles/r5/split2_tails_f.jsonl): torus roles ending at 439 / 378 / 436 us with
    // geometric shares, 440 / 417 / 430 with 0.68 / 0.76.  Both retunes were measured on single boards only, so the
    // ghost-row strips of N > 1 keep round 4's measured split on either boundary (`single`: one strip holding the whole
    // board, ghost 0): torus strips fall through to 0.70 below, bounded strips keep 0.64.
    if (bounded && ilv == 2 && k == 12) return (int)((single ? 0.60 : 0.64) * 65536);
    if (!bounded && wrap && ilv == 2 && k == 12) return (int)(0.66 * 65536);
    // measured at 65536^2 (profiles/r1/split_sweep*.log, two boxes): the deep passes gain 3-9 %; the
    // shallow ones (short, memory-bound trips) are left unpaired
    // (12, 2) runs 12-wave workgroups at 3 waves/SIMD: three-way groups (profiles/r1/w12_sweep*.log)
    // Round 3, staged passes, fresh 65536^2 board, forward + reverse sweep (profiles/r3/split_sweep_f.log): torus
    // (12, 2) 0.64 / 0.68 / 0.72 -> 95.9k / 96.8k / 95.0k; torus (16, 2) 0.60 / 0.64 / 0.68 / 0.72 -> 101.8k / 107.5k /
    // 107.6k / 104.7k; bounded (12, 2) 0.60 / 0.64 / 0.68 -> 96.6k / 99.0k / 95.4k; bounded (16, 2) 0.56 / 0.60 /
    // 0.64 / 0.68 -> 112.5k / 112.0k / 106.2k / 100.7k (a slope now, not round 2's cliff).
    if (bounded && ilv == 2 && k == 16) return (int)(0.60 * 65536);
    // (bounded (12, 2): 0.64 until round 5, above)
    if (ilv == 1 && k >= 24) return (int)(0.60 * 65536);
    if (ilv == 2 && k == 12) return (int)(0.70 * 65536);
    if (ilv == 2 && k >= 16) return (int)(0.66 * 65536);
    if (ilv == 4 && k >= 8) return (int)(0.55 * 65536);
    return 0;
}

// Remainder units of the seam geometry for nsegs segments (kernel: the unit mapping in gol_stream_step).
static int64_t seam_rem_units(const StreamArgs& a, int64_t nsegs, int64_t rem_mid) {
    if (!a.seam || a.rem == 0 || nsegs <= 0) return 0;
    return 1 + (rem_mid + a.rem_p - 1) / a.rem_p + (nsegs - 1 - rem_mid);
}

// Does the seam geometry apply?  Torus deep passes (the bounded edge-fill strips keep their zero-fill edges) on rows
// of at least one seam strip, with K <= 16 M (the break in the middle of the seam lane must not reach its ends).
static bool seam_applies(const StreamArgs& a, int k, bool bounded) {
    return a.seam_opt >= 0 && !bounded && !a.rag_bits && k > 1 && k <= 16 * a.ilv && a.words / a.ilv >= kSeamInterior;
}

// Three-wave groups: the middle wave's share of the two younger waves' rows (1/65536), 0 = geometric.
int stream_split2(int k, int ilv, bool bounded, bool wrap, bool single) {
    if (kWavesPerBlock < 8 || ilv != 2 || k != 12 || !single) return 0;  // (12, 2) single boards: see stream_pair_split
    if (bounded) return (int)(0.72 * 65536);
    return wrap ? (int)(0.76 * 65536) : 0;
}

// Work decomposition: nstrips column strips x nsegs row segments, one wave each (or one SIMD group of
// waves per segment with the pair split), plus the seam geometry's remainder units.  The segment count makes the
// grid ONE balanced round of resident waves (a partial second round would leave a tail of lone waves), with
// segments no shorter than 2K rows (pipeline fill cost).  a.split_opt / a.seg_opt / a.seam_opt (a board's "split" /
// "seg_rows" / "seam" options) override the split, the segment length and the geometry for experiments.
void plan_stream(StreamArgs& a, int k, bool bounded, bool wrap) {
    const bool single = a.ghost == 0 && a.rows == a.height;  // the whole board in one buffer (not a ghost-row strip)
    a.split = a.split_opt > 0 ? a.split_opt : (a.split_opt < 0 ? 0 : stream_pair_split(k, a.ilv, bounded, wrap, single));
    a.split2 = a.split2_opt > 0 ? a.split2_opt : stream_split2(k, a.ilv, bounded, wrap, single);
    const int64_t nblocks = a.words / a.ilv;
    a.seam = seam_applies(a, k, bounded) ? 1 : 0;
    a.rem = 0;
    a.rem_p = 1;
    a.rem_units = 0;
    a.rem_mid = 0;
    if (a.seam) {
        a.nstrips = nblocks / kSeamInterior;
        a.rem = (int32_t)(nblocks - a.nstrips * kSeamInterior);
        a.rem_p = a.rem ? (kWave / (a.rem + 2) > 0 ? kWave / (a.rem + 2) : 1) : 1;
    } else {
        a.nstrips = stream_strips(a.words, a.ilv, k, bounded, a.rag_bits);
    }
    // Ragged torus rows (StreamWave kRagged): the strips start at ring position -1 (the partial last word, then word
    // 0, ...), unless the last strip's right halo lane would then be the partial word next to a stored word; then
    // at position -2.
    a.rag_origin = 1;
    if (a.rag_bits && !bounded && (a.nstrips * kInterior - 1 + 1) % nblocks == 0) a.rag_origin = 2;
    const int64_t rows = a.out_end - a.out_begin;
    if (rows <= 0) {
        a.nsegs = 0;
        a.seg = 1;
        return;
    }
    // a launch too short for one full group segment per strip (e.g. a k-row halo band) runs one wave per
    // segment: splitting a handful of rows only multiplies the pipeline fill
    const int wpb = stream_wpb(a.words, k, a.ilv, bounded, wrap, a.rag_bits);
    if (a.split && rows < (int64_t)(wpb / 4) * (2 * k > 16 ? 2 * k : 16)) a.split = 0;
    const int group = a.split ? wpb / 4 : 1;  // waves per segment
    int64_t seg = a.seg_opt;
    int64_t slots = 0;
    if (seg <= 0) {
        int64_t units = resident_units(a.words, k, a.ilv, bounded, wrap, a.rag_bits);
        if (a.spare > 0) units = units > a.spare + 1 ? units - a.spare : 1;
        slots = units / group;
        // waves per segment: the strips, plus (seam geometry) a 1/rem_p share of a remainder wave
        const double per_seg = (double)a.nstrips + (a.seam && a.rem ? 1.0 / a.rem_p : 0.0);
        int64_t nsegs = (int64_t)((double)slots / per_seg);
        if (nsegs < 1) nsegs = 1;
        int64_t min_seg = (2 * k > 16 ? 2 * k : 16) * group;
        // A launch too small to fill a quarter of the device is latency-bound: each wave is one serial
        // chain of (segment + 2k) rows x k levels, so shorter segments (more, shorter chains) finish sooner
        // despite the extra pipeline fill.  1024^2: 549 -> 696 GCUPS, 4096^2: 8.7k -> 10.5k at K = 8, ilv 1
        // (profiles/r1/small_seg.log).  Large boards are bounded by `slots` below and do not change.
        if ((rows / min_seg) * a.nstrips * group < units / 4) min_seg = (k > 8 ? k : 8) * group;
        const int64_t max_segs = rows / min_seg > 0 ? rows / min_seg : 1;
        if (nsegs > max_segs) nsegs = max_segs;
        seg = (rows + nsegs - 1) / nsegs;
    }
    if (seg > ((int64_t)1 << 30)) seg = (int64_t)1 << 30;  // the kernel counts a segment's rows in 32 bits
    a.seg = seg;
    a.nsegs = (rows + seg - 1) / seg;
    if (a.seam && a.rem) {
        // the per-lane row offsets of a packed remainder wave are 32-bit byte offsets into one descriptor
        const int64_t row_bytes = a.words * 4, step = seg * (a.pitch > 0 ? a.pitch : a.words) * 4;
        const int64_t fit = 1 + ((((int64_t)1 << 31) - 1 - row_bytes) / step);
        if (a.rem_p > fit) a.rem_p = (int32_t)(fit > 1 ? fit : 1);
        // segments 1 .. rem_mid share remainder waves: every row they stream must lie in the board / buffer
        // without a wrap.  Sub-strip j reads its rows at a fixed offset from sub-strip 0's walk, which wraps (single
        // board) or clamps (ghost-row strip) only for itself; so the last packed segment's rows -- its k halo rows
        // below and the walk's overshoot -- must end inside the buffer.  The walk prefetches whole trips of R = 4
        // rows, one trip ahead, and the last trip prefetches one more (unused): ceil((seg + 2k) / 4) + 1 trips, up to
        // 7 rows past the seg + 2k the segment streams.  Round 3 let those rows run past the buffer's end: reads
        // beyond the allocation, harmless unless the next page was unmapped -- an illegal-address fault in round 4's
        // suite on an 8209 x 40 ragged board (ring rows of 262 words, 42 KB), found by the GOL_CHECK_BOUNDS build
        // (descriptor tag 8) and reproduced on the CPU by walking the plan.
        const int64_t trip = kDeepTripRows;  // TripRows of every seam pass (K > 1)
        const int64_t over = ((seg + 2 * k + trip - 1) / trip + 1) * trip - (seg + 2 * k);
        const int64_t limit = wrap ? a.rows : a.rows + a.ghost;  // first row index past the buffer (owned-row units)
        int64_t mid = a.nsegs - 2;
        const int64_t fit_mid = (limit - a.out_begin - k - over) / seg - 1;  // (m + 1) seg + k + over <= limit - out_begin
        if (fit_mid < mid) mid = fit_mid;
        // sub-strip j streams rows [(j + 1) seg - k, (j + 2) seg + k) of the buffer at a fixed offset from
        // sub-strip 0's walk: a segment shorter than k (the "seg_rows" option can ask for one) would make segment 1's
        // first rows wrap or leave the buffer, so such segments run as lone remainder units
        if (seg < k) mid = 0;
        a.rem_mid = mid > 0 ? mid : 0;
        a.rem_units = seam_rem_units(a, a.nsegs, a.rem_mid);
    }
}

PipeArgs pipe_args(const StreamArgs& a, bool bounded) {
    PipeArgs p{};
    p.words = a.words;
    p.pitch = a.pitch;
    p.rows = a.rows;
    p.ghost = a.ghost;
    p.out_begin = a.out_begin;
    p.out_end = a.out_end;
    p.split1 = a.pipe_split_opt;
    p.split2 = a.pipe_split2_opt;
    p.spare_waves = a.spare;
    p.err = a.pipe_err ? a.pipe_err : pipe_error_word();
    p.bounded = bounded ? 1 : 0;
    if (bounded) {  // the board's rows in owned-row coordinates, clipped to the buffer (Script.fsx:6-13)
        const int64_t lo = -a.y0 > -a.ghost ? -a.y0 : -a.ghost;
        const int64_t hi = a.height - a.y0 < a.rows + a.ghost ? a.height - a.y0 : a.rows + a.ghost;
        p.live_lo = (int32_t)lo;
        p.live_hi = (int32_t)hi;
    }
    return p;
}

}  // namespace gol
