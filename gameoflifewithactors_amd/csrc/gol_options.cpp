// gol_options.cpp -- the ONE table of a board's options: gol_set_option / gol_get_option (include/gol/gol.h) and the
// test and A/B knobs of gol_debug_set_option / gol_debug_get_option (gol_debug.h) are rows of it, told apart by a flag.
// gol_debug_option_names() is generated from it; the fields and their meaning are BoardOptions (gol_board.h).
#include "gol_board.h"
#include "gol_debug.h"

namespace gol {
namespace {

enum : int { kDebug = 1, kMultiOnly = 2 };  // a gol_debug.h knob; only a multi-part board takes a set

struct Option {
    const char* name;
    int flags;
    int64_t (*get)(const gol_board* b);
    int (*set)(gol_board* b, int64_t value);  // validates, normalises, stores; nullptr: read-only
};

// Getter and the two plain setters of a BoardOptions field: any value, or a flag (non-zero = on)
using O = BoardOptions;
template <auto M>
int64_t get(const gol_board* b) {
    return (int64_t)(b->opt.*M);
}
template <auto M>
int set_any(gol_board* b, int64_t v) {
    b->opt.*M = v;
    return GOL_OK;
}
template <auto M>
int set_flag(gol_board* b, int64_t v) {
    b->opt.*M = v != 0;
    return GOL_OK;
}
// value in [lo, hi], or GOL_ERR_INVALID with `msg`
template <class T>
int set_in(T& field, int64_t v, int64_t lo, int64_t hi, const std::string& msg) {
    if (v < lo || v > hi) return fail(GOL_ERR_INVALID, msg);
    field = (T)v;
    return GOL_OK;
}
// a 1/65536 ratio: below 65536, every negative value stored as -1
int set_ratio(int32_t& field, int64_t v, const std::string& msg) { return set_in(field, v < 0 ? -1 : v, -1, 65535, msg); }

const Option kOptions[] = {
    {"coop", 0, get<&O::coop>, set_flag<&O::coop>},
    {"coop_k", 0, get<&O::coop_k>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.coop_k, v, 0, 64, "coop_k must be 0 (default) .. 64"); }},
    {"coop_max_cells", 0, get<&O::coop_max_cells>, set_any<&O::coop_max_cells>},
    {"resident_max_cells", 0, get<&O::resident_max_cells>, set_any<&O::resident_max_cells>},
    {"wave_resident", 0, get<&O::wave_resident>, set_flag<&O::wave_resident>},
    {"split", 0, get<&O::split>,
     [](gol_board* b, int64_t v) { return set_ratio(b->opt.split, v, "split must be < 65536 (1/65536 units; 0 default, < 0 off)"); }},
    {"split2", 0, get<&O::split2>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.split2, v, 0, 65535, "split2 must be 0 (engine) .. 65535 (1/65536 units)"); }},
    {"seg_rows", 0, get<&O::seg_rows>, [](gol_board* b, int64_t v) { return set_any<&O::seg_rows>(b, v < 0 ? 0 : v); }},
    {"seam", 0, get<&O::seam>, [](gol_board* b, int64_t v) { return set_any<&O::seam>(b, v < 0 ? -1 : 0); }},
    {"pipe_split", 0, get<&O::pipe_split>,
     [](gol_board* b, int64_t v) { return set_ratio(b->opt.pipe_split, v, "pipe_split must be < 65536 (1/65536 units; 0 default, < 0 equal)"); }},
    {"pipe_split2", 0, get<&O::pipe_split2>,
     [](gol_board* b, int64_t v) { return set_ratio(b->opt.pipe_split2, v, "pipe_split2 must be < 65536 (1/65536 units; 0 default, < 0 equal)"); }},
    // multi-part boards: 1 = peer copies (the default), 2 = RCCL (distinct devices only)
    {"transport", kMultiOnly,
     [](const gol_board* b) -> int64_t { return b->multi ? b->multi->transport() : GOL_TRANSPORT_NONE; },
     [](gol_board* b, int64_t v) { return b->multi->set_transport((int)v); }},
    {"ragged_stream", 0, get<&O::ragged_stream>, set_flag<&O::ragged_stream>},
    {"ragged_ring", 0, get<&O::ragged_ring>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.ragged_ring, v, 0, 2, "ragged_ring must be 0, 1 (by size) or 2"); }},
    {"coop_poll_delay", 0, get<&O::coop_poll_delay>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.coop_poll_delay, v, -1, 4096, "coop_poll_delay must be -1 (auto) or 0..4096"); }},
    {"lanes", 0, get<&O::lanes>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.lanes, v, 0, 2, "lanes must be 0, 1 or 2 (by size)"); }},
    {"lanes_m", 0, get<&O::lanes_m>,
     [](gol_board* b, int64_t v) {
         if (v != 0 && v != 3 && v != 5 && v != 9 && v != 17) return fail(GOL_ERR_INVALID, "lanes_m must be 0, 3, 5, 9 or 17");
         return set_any<&O::lanes_m>(b, v);
     }},
    {"view_stream", 0, get<&O::view_stream>, set_flag<&O::view_stream>},
    {"rule_ragged", 0, get<&O::rule_ragged>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.rule_ragged, v, 0, 2, "rule_ragged must be 0, 1 (by size and call length) or 2"); }},
    // ---- test and A/B knobs (gol_debug.h)
    {"coop_epoch", kDebug, [](const gol_board* b) -> int64_t { return b->coop_epoch; },
     [](gol_board* b, int64_t v) {
         // the epoch of the last persistent launch, so the next one runs at value + 1: tests run the 16-bit wrap early.
         // The granules are cleared with it: the buffer may hold granules of any earlier
         // epoch, among them value + 1's own block 0 of parity 0, which would otherwise match the next launch's first
         // poll and hand it stale halo rows.
         if (v < 0 || v > 0xffff) return fail(GOL_ERR_INVALID, "coop_epoch must be 0..65535");
         if (b->coop_xch) {
             GOL_HIP(hipMemsetAsync(b->coop_xch, 0, (size_t)b->coop_xch_words * sizeof(uint32_t), b->stream));
             b->coop_epoch = (unsigned)v;
         }
         return GOL_OK;
     }},
    {"coop_spin_limit", kDebug, get<&O::coop_spin_limit>,
     [](gol_board* b, int64_t v) { return set_any<&O::coop_spin_limit>(b, v < 0 ? 0 : v); }},
    {"coop_r", kDebug, get<&O::coop_r>,
     [](gol_board* b, int64_t v) { return set_in(b->opt.coop_r, v, 1, 8, "coop_r must be 1..8"); }},
    {"resident_threads", kDebug, get<&O::resident_threads>,
     [](gol_board* b, int64_t v) {
         if (v != 256 && v != 1024) return fail(GOL_ERR_INVALID, "resident_threads must be 256 or 1024");
         return set_any<&O::resident_threads>(b, v);
     }},
    {"coop_launch", kDebug, get<&O::coop_launch>, set_flag<&O::coop_launch>},
    {"lanes_launches", kDebug, [](const gol_board* b) -> int64_t { return b->lanes_launches; }, nullptr},
    {"last_pass", kDebug, [](const gol_board* b) -> int64_t { return (int64_t)b->last_pass; }, nullptr},
    {"rule_table", kDebug, get<&O::rule_table>,
     [](gol_board* b, int64_t v) {
         if (v != 0 && v != 1) return fail(GOL_ERR_INVALID, "rule_table must be 0 or 1");
         if (v && b->multi) return fail(GOL_ERR_UNSUPPORTED, "rule_table: a multi-part board runs B3/S23 on its strip passes only");
         // no ragged multi-generation pass runs in the rule family: the bytes first (as gol_set_rule)
         if (!b->multi) GOL_RC(sync_bytes(b));
         return set_flag<&O::rule_table>(b, v);
     }},
    {"rule_k", kDebug, get<&O::rule_k>,
     [](gol_board* b, int64_t v) {
         if (v != 0 && v != 1 && v != 2 && v != 4 && v != 8) return fail(GOL_ERR_INVALID, "rule_k must be 0, 1, 2, 4 or 8");
         if (v == 8 && b->nstates > 2)
             return fail(GOL_ERR_INVALID, "rule_k 8: a Generations board's streaming pass runs 4, 2 or 1 generations per pass");
         return set_any<&O::rule_k>(b, v);
     }},
    {"rule_seg_rows", kDebug, get<&O::rule_seg_rows>,
     [](gol_board* b, int64_t v) { return set_any<&O::rule_seg_rows>(b, v < 0 ? 0 : v); }},
};

// One option call: reads into *value (`get`) or stores it.  `debug`: through the gol_debug_* entry points, which know
// the knobs only, as gol_set_option / gol_get_option know the board options only.
int option_call(gol_board* b, const char* name, bool debug, bool get, int64_t* value) {
    return with_board(b, [&] {
        if (!name || !value) return fail(GOL_ERR_INVALID, get ? "null argument" : "null option name");
        const std::string n(name);
        for (const Option& o : kOptions) {
            if (n != o.name) continue;
            if (debug != ((o.flags & kDebug) != 0)) {
                if (debug) break;
                return fail(GOL_ERR_INVALID, "'" + n + "' is a test knob (gol_debug_" + (get ? "get" : "set") +
                                                 "_option, csrc/gol_debug.h), not a board option");
            }
            if (get) {
                *value = o.get(b);
                return GOL_OK;
            }
            if (!o.set) return fail(GOL_ERR_INVALID, n + " is read-only");
            if ((o.flags & kMultiOnly) && !b->multi)
                return fail(GOL_ERR_UNSUPPORTED, n + ": a single board has no halo exchange");
            GOL_RC(o.set(b, *value));
            // a multi-part board runs every strip launch with the streaming options (the other passes never run there)
            if (b->multi) b->multi->set_stream_options(b->opt.split, b->opt.seg_rows, b->opt.seam, b->opt.split2);
            return GOL_OK;
        }
        return fail(GOL_ERR_INVALID, std::string(debug ? "unknown debug option '" : "unknown option '") + n + "'");
    });
}

}  // namespace
}  // namespace gol

extern "C" {

int gol_set_option(gol_board* b, const char* name, int64_t value) { return gol::option_call(b, name, false, false, &value); }
int gol_get_option(gol_board* b, const char* name, int64_t* value) { return gol::option_call(b, name, false, true, value); }

// Test and A/B knobs (csrc/gol_debug.h; VERDICT round 4 item 3: kept out of gol.h's option list).
int gol_debug_set_option(gol_board* b, const char* name, int64_t value) { return gol::option_call(b, name, true, false, &value); }
int gol_debug_get_option(gol_board* b, const char* name, int64_t* value) { return gol::option_call(b, name, true, true, value); }

const char* gol_debug_option_names(void) {
    static const std::string names = [] {
        std::string r;
        for (const gol::Option& o : gol::kOptions)
            if (o.flags & gol::kDebug) r += (r.empty() ? "" : ",") + std::string(o.name);
        return r;
    }();
    return names.c_str();
}

}  // extern "C"
