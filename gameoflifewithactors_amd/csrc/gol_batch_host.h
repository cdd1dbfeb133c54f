// gol_batch_host.h -- the host-only arithmetic of the batch handle (gol_batch.cpp): argument ranges, the .NET seeding
// of packed boards and the per-board rule table; a batch's geometry is the single-wave pass's (gol_wave_shape.h
// wave_resident_rpl).  No HIP here, so tests/cpp/test_batch_host.cpp and tests/cpp/test_batch_rules_host.cpp compile
// it alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include "gol_rule.h"
#include "gol_seed_rle.h"
#include "gol_wave_shape.h"

namespace gol {

constexpr int64_t kBatchCountMax = (int64_t)1 << 22;  // boards per batch
constexpr int64_t kBatchTraceMax = (int64_t)1 << 26;  // entries of one gol_batch_step_trace call

// Boards [first, first + n) lie inside [0, count) and `len` is their n * cells bytes (n >= 1; no overflow for any input).
inline bool batch_range_ok(int64_t first, int64_t n, int64_t count, int64_t len, int64_t cells) {
    if (first < 0 || n < 1 || first >= count || n > count - first) return false;
    return len == n * cells;  // n <= 2^22 and cells <= 2^15
}

// A trace call: generations >= 0 a multiple of every >= 1, generations / every samples of `count` entries each, at most
// kBatchTraceMax in all, len exactly that many.  *samples is set when the call is valid.
inline bool batch_trace_ok(int64_t generations, int64_t every, int64_t count, int64_t len, int64_t* samples,
                           const char** why) {
    if (generations < 0) return *why = "generations must be >= 0", false;
    if (every < 1) return *why = "every must be >= 1", false;
    if (generations % every) return *why = "generations must be a multiple of every", false;
    const int64_t t = generations / every;
    if (t > kBatchTraceMax / count) return *why = "more than 2^26 trace entries", false;
    if (len != t * count) return *why = "trace length must be (generations / every) * count", false;
    *samples = t;
    return true;
}

// A per-board rule table (gol_ensemble_set_rules): n == count entries, both arrays there, every mask in 0..0x1FF.  The
// whole table is judged before a word of `packed` is written: true with packed[i] = rule_pack(birth[i], survive[i])
// for i in [0, count), or false with *why set and `packed` untouched.  *bad_index, when given, is the first entry
// with a mask out of range, or -1.
inline bool batch_rules_pack(const int* birth, const int* survive, int64_t n, int64_t count, uint32_t* packed,
                             const char** why, int64_t* bad_index = nullptr) {
    if (bad_index) *bad_index = -1;
    if (!birth || !survive) return *why = "birth and survive must hold count entries: null array", false;
    if (n != count) return *why = "birth and survive must hold count entries", false;
    if (!packed) return *why = "null table", false;
    for (int64_t i = 0; i < n; i++)
        if (!rule_masks_ok(birth[i], survive[i])) {
            if (bad_index) *bad_index = i;
            return *why = "birth and survive masks must lie in 0..0x1FF", false;
        }
    for (int64_t i = 0; i < n; i++) packed[i] = rule_pack(birth[i], survive[i]);
    return true;
}

// The rule every entry of a packed table agrees on (count >= 1): true with *rule set, or false with *rule untouched.
inline bool batch_rules_common(const uint32_t* packed, int64_t count, uint32_t* rule) {
    for (int64_t i = 1; i < count; i++)
        if (packed[i] != packed[0]) return false;
    *rule = packed[0];
    return true;
}

// The packed rows (nw = ceil(W / 32) words each) of the board gol_seed_dotnet(seed, mode) makes: creation order x outer,
// y inner (GameOfLifeDriver.fs:16-19; Array2D.init in Script.fsx:27); mode 0: Next() % 2 = 0, mode 1: Next(2) = 0.
inline void batch_seed_dotnet_words(int32_t seed, int mode, int64_t W, int64_t H, uint32_t* words) {
    const int64_t nw = (W + 31) / 32;
    for (int64_t k = 0; k < nw * H; k++) words[k] = 0;
    DotNetRandom r(seed);
    for (int64_t x = 0; x < W; x++)
        for (int64_t y = 0; y < H; y++) {
            const bool alive = mode == 0 ? (r.Next() % 2 == 0) : (r.Next(2) == 0);
            if (alive) words[y * nw + (x >> 5)] |= 1u << (x & 31);
        }
}

}  // namespace gol
