// gol_passes.cpp -- stepping: gol_step, gol_step_timed and gol_pass_timing run the pass the policy picks for the call
// (gol_policy.cpp choose_pass), one small executor per pass, each a chunk rule and a launch on the shared ping-pong
// loop.  A ragged byte board's scratch-row state (gol_board::rag_state) is settled between the choice and the pass.
#include <algorithm>

#include "gol_board.h"
#include "gol_gen_plan.h"

using gol::check_valid;
using gol::fail;
using gol::kCoopErrWord;
using gol::kCoopFlagWords;
using gol::Pass;
using gol::sync_bytes;
using gol::with_board;

namespace {

constexpr int64_t kResidentMaxGensPerLaunch = (int64_t)1 << 16;
constexpr int64_t kCoopMaxGensPerLaunch = 32768;  // a launch's granule tags count its blocks in 16 bits
constexpr int kRingCopy = 64;  // cells copied at each end of a ring row (gol_formats.hip kRingPad; the suffix has >= 64)

// The board's error word (b->coop[kCoopErrWord]): the persistent passes' timed-out hand-offs and the level-pipelined
// pass's timed-out ring waits (check_valid)
int ensure_err_word(gol_board* b) {
    if (!b->coop) {
        GOL_HIP(hipMalloc(&b->coop, kCoopFlagWords * sizeof(unsigned)));
        GOL_HIP(hipMemsetAsync(b->coop, 0, kCoopFlagWords * sizeof(unsigned), b->stream));
    }
    return GOL_OK;
}

// The loop of every pass: `gens` generations as launches of chunk(generations left) generations each, ping-ponging
// between two buffers -- launch(g) reads buffer *cur and writes buffer *cur ^ 1; *cur ends on the result.
template <class Chunk, class Launch>
int ping_pong(gol_board* b, int* cur, int64_t gens, Chunk chunk, Launch launch) {
    while (gens > 0) {
        const int64_t g = chunk(gens);
        GOL_RC(launch(g));
        *cur ^= 1;
        b->generation += g;
        gens -= g;
    }
    return GOL_OK;
}
// the chunk rule of the passes that run any number of generations in one launch: at most `cap` of them
auto at_most(int64_t cap) {
    return [cap](int64_t left) { return std::min(left, cap); };
}

// `gens` generations of the cooperative pass on packed rows of W cells (`pitch` words, layout `ilv`; ragged_w > 0:
// scratch rows of a ragged board of that width), ping-ponging between bufs[*cur] and bufs[*cur ^ 1]; *cur ends on
// the result.  One launch per kCoopMaxGensPerLaunch generations.
int coop_steps(gol_board* b, int64_t W, int64_t pitch, int ilv, int64_t ragged_w, uint32_t* const bufs[2], int* cur,
               int64_t gens, bool lanes = false) {
    GOL_RC(ensure_err_word(b));
    int nwg = 0, B = 0, R = 0;
    const int k = lanes ? gol::lanes_depth(b) : gol::coop_depth(b);
    int64_t need = 0;
    if (lanes) {
        gol::LanesPlan lp;
        (void)gol::lanes_plan(W, b->H, k, b->opt.lanes_m, &lp);
        need = gol::lanes_xch_words(lp, k);
    } else {
        (void)gol::coop_plan(W, b->H, k, &nwg, &B, &R, b->opt.coop_r);
        need = gol::coop_xch_words(W, nwg, k);
    }
    if (need > b->coop_xch_words) {
        if (b->coop_xch) {
            GOL_HIP(hipStreamSynchronize(b->stream));
            GOL_HIP(hipFree(b->coop_xch));
            b->coop_xch = nullptr;
            b->coop_xch_words = 0;
        }
        GOL_HIP(hipMalloc(&b->coop_xch, (size_t)need * sizeof(uint32_t)));
        b->coop_xch_words = need;
        b->coop_epoch = 0xffff;  // forces the clear below: a fresh buffer holds arbitrary tags
    }
    gol::CoopTuning tune;
    tune.min_rows = b->opt.coop_r;
    // first-poll delay (s_sleep periods, 64 clocks each), measured after the error word left the hand-off's critical
    // path (profiles/r5/coop_delay_ab_m.log, us/generation): 4096-wide rows poll at once (4096^2 0.535 at 0 / 0.537 at 4
    // / 0.548 at 8), narrower rows after 4 (1024^2 0.447 against 0.453 at 0; 2048 x 1024 0.383 against 0.385; 2048^2
    // 0.408 against 0.409), 8192-wide rows after 24 (8192 x 4096 1.09 against 1.11 at 40 and 1.16 at 64); the
    // rows-on-lanes pass keeps 8 (256^2 bounded 0.253 against 0.253 at 0 and 0.268 at 16; lanes_small_m.log)
    tune.poll_delay = b->opt.coop_poll_delay >= 0 ? b->opt.coop_poll_delay : (lanes ? 8 : (W < 4096 ? 4 : (W == 4096 ? 0 : 24)));
    tune.spin_limit = (unsigned)std::min<int64_t>(b->opt.coop_spin_limit, 0xffffffffLL);
    tune.plain_launch = !b->opt.coop_launch;
    int* const err = reinterpret_cast<int*>(b->coop + kCoopErrWord);
    const bool bounded = b->boundary == GOL_BOUNDED;
    return ping_pong(b, cur, gens, at_most(kCoopMaxGensPerLaunch), [&](int64_t g) {
        if (++b->coop_epoch > 0xffff) {  // tags of an earlier epoch could match again: clear the granules
            GOL_HIP(hipMemsetAsync(b->coop_xch, 0, (size_t)b->coop_xch_words * sizeof(uint32_t), b->stream));
            b->coop_epoch = 1;
        }
        if (lanes) {
            ++b->lanes_launches;
            GOL_HIP(gol::launch_lanes_pass(bufs[*cur], bufs[*cur ^ 1], W, b->H, pitch, ilv, k, g, bounded, b->coop_epoch,
                                           err, b->coop_xch, b->coop_xch_words, b->stream, b->opt.lanes_m, tune));
        } else {
            GOL_HIP(gol::launch_coop_pass(bufs[*cur], bufs[*cur ^ 1], W, b->H, pitch, ilv, k, g, bounded, b->coop_epoch,
                                          err, b->coop_xch, b->coop_xch_words, b->stream, ragged_w, tune));
        }
        return GOL_OK;
    });
}

// Whole-word scratch rows for a ragged byte board (two buffers of `need` words).
int ensure_rag(gol_board* b, int64_t need) {
    if (need <= b->rag_words) return GOL_OK;
    GOL_HIP(hipStreamSynchronize(b->stream));
    for (uint32_t*& r : b->rag) {
        if (r) GOL_HIP(hipFree(r));
        r = nullptr;
    }
    b->rag_words = 0;
    for (uint32_t*& r : b->rag) {
        const hipError_t e = hipMalloc(&r, (size_t)need * sizeof(uint32_t));
        if (e != hipSuccess) {
            r = nullptr;
            return fail(GOL_ERR_OOM, std::string("hipMalloc ragged scratch: ") + hipGetErrorString(e));
        }
    }
    b->rag_words = need;
    return GOL_OK;
}

// ---------------------------------------------------------------- one executor per pass (gol::Pass)
int run_wave(gol_board* b, int64_t gens) {
    return ping_pong(b, &b->cur, gens, at_most(kResidentMaxGensPerLaunch), [&](int64_t g) {
        GOL_HIP(gol::launch_wave_resident(b->buf[b->cur], b->buf[b->cur ^ 1], b->W, b->H, b->pitch, g,
                                          b->boundary == GOL_BOUNDED, !b->packed, b->rule, b->opt.rule_table, b->stream));
        return GOL_OK;
    });
}

int run_coop(gol_board* b, int64_t gens, bool lanes) {
    uint32_t* bufs[2] = {b->words(0), b->words(1)};
    return coop_steps(b, b->W, b->pitch, b->ilv, 0, bufs, &b->cur, gens, lanes);
}

// the ragged byte board as whole words in scratch rows (packed once, kept there after the call), the pass
int run_coop_ragged(gol_board* b, int64_t gens, int64_t rag_pitch) {
    if (b->rag_state != 2) {
        GOL_RC(ensure_rag(b, rag_pitch * b->H));
        GOL_HIP(gol::launch_pack_ragged(b->cells(b->cur), b->rag[0], b->W, b->H, rag_pitch, b->stream));
        b->rag_cur = 0;
    }
    int rc_cur = b->rag_cur;
    const int rc = coop_steps(b, rag_pitch * 32, rag_pitch, 1, b->W, b->rag, &rc_cur, gens);
    b->rag_state = 2;
    b->rag_cur = rc_cur;
    b->rag_pitch = rag_pitch;
    return rc;
}

// the ragged board as block rows (packed once, kept there after the call), the aligned streaming kernel
int run_ring(gol_board* b, int64_t gens) {
    const bool torus = b->boundary == GOL_TORUS;
    const int64_t pitch = gol::ring_pitch(b->W, torus);
    const int ilv = gol::ring_ilv(b);
    if (b->rag_state != 3) {
        GOL_RC(ensure_rag(b, pitch * b->H));
        GOL_HIP(gol::launch_pack_ring(b->cells(b->cur), b->rag[0], b->W, b->H, ilv, torus, b->stream));
        b->rag_cur = 0;
        b->ring_age = 0;
    }
    b->rag_state = 3;
    b->rag_pitch = pitch;
    b->rag_ilv = ilv;
    auto depth = [&](int64_t left) { return (int64_t)gol::stream_largest_k(left, b->tblock, ilv); };
    return ping_pong(b, &b->rag_cur, gens, depth, [&](int64_t g) {
        const int k = (int)g;
        gol::StreamArgs a = b->stream_args(0, b->H, k);
        a.words = pitch;
        a.pitch = pitch;
        a.ilv = ilv;
        if (!torus) {  // cells past the row's end stay dead (column masks)
            a.rag_bits = (int32_t)(b->W % 32);
            a.rag_w = b->W;
        }
        // ring rows: the errors from the extended row's ends spread k cells per pass; refresh the copies before
        // a pass would carry them past the 64 copied cells into the board's own
        if (torus && b->ring_age + k > kRingCopy) {
            GOL_HIP(gol::launch_ring_refresh(b->rag[b->rag_cur], b->W, b->H, ilv, b->stream));
            b->ring_age = 0;
        }
        GOL_HIP(gol::launch_stream_step(b->rag[b->rag_cur], b->rag[b->rag_cur ^ 1], a, k, !torus, torus, b->stream));
        b->ring_age += k;
        return GOL_OK;
    });
}

// the ragged byte board as whole words in scratch rows (packed once, kept there after the call), streaming
int run_stream_ragged(gol_board* b, int64_t gens) {
    const int64_t nw = (b->W + 31) / 32;
    if (b->rag_state != 1) {
        GOL_RC(ensure_rag(b, nw * b->H));
        GOL_HIP(gol::launch_pack_ragged(b->cells(b->cur), b->rag[0], b->W, b->H, nw, b->stream));
        b->rag_cur = 0;
    }
    b->rag_state = 1;
    b->rag_pitch = nw;
    // a ragged board's default depth is the block rows' (board_layout); this M = 1 path keeps its own
    const int cap = b->tblock_set ? b->tblock : gol::board_tblock(0, b->W * b->H, b->boundary);
    auto depth = [&](int64_t left) { return (int64_t)gol::stream_largest_k(left, cap, 1); };
    return ping_pong(b, &b->rag_cur, gens, depth, [&](int64_t g) {
        const int k = (int)g;
        gol::StreamArgs a = b->stream_args(0, b->H, k);
        a.words = nw;
        a.pitch = nw;
        a.ilv = 1;
        a.rag_bits = (int32_t)(b->W % 32);
        a.rag_w = b->boundary == GOL_BOUNDED ? b->W : 0;
        GOL_HIP(gol::launch_stream_step(b->rag[b->rag_cur], b->rag[b->rag_cur ^ 1], a, k, b->boundary == GOL_BOUNDED,
                                        b->boundary == GOL_TORUS, b->stream));
        return GOL_OK;
    });
}

int run_resident(gol_board* b, int64_t gens) {
    const bool bounded = b->boundary == GOL_BOUNDED;
    // one launch per 2^16 generations (a few tens of ms): a long gol_step stays interruptible by
    // readbacks and other work on the board's stream
    return ping_pong(b, &b->cur, gens, at_most(kResidentMaxGensPerLaunch), [&](int64_t g) {
        if (b->packed)
            GOL_HIP(gol::launch_resident_packed(b->words(b->cur), b->words(b->cur ^ 1), b->W, b->H, b->pitch, g, bounded,
                                                b->stream, b->opt.resident_threads));
        else
            GOL_HIP(gol::launch_resident_bytes(b->cells(b->cur), b->cells(b->cur ^ 1), b->W, b->H, g, bounded, b->stream,
                                               b->opt.resident_threads));
        return GOL_OK;
    });
}

int run_bytes(gol_board* b, int64_t gens) {
    const bool rule = b->rule_family();
    return ping_pong(b, &b->cur, gens, at_most(1), [&](int64_t) {
        if (b->nstates > 2)  // a Generations board: the (alive byte, d byte) pair, both ping-ponging
            GOL_HIP(gol::launch_bytes_gen_step(b->cells(b->cur), b->dec_cells(b->cur), b->cells(b->cur ^ 1),
                                               b->dec_cells(b->cur ^ 1), b->W, b->H, b->boundary == GOL_BOUNDED,
                                               (int)(b->rule & 0x1FF), (int)(b->rule >> 9), b->nstates, b->stream));
        else if (rule)
            GOL_HIP(gol::launch_bytes_rule_step(b->cells(b->cur), b->cells(b->cur ^ 1), b->W, b->H,
                                                b->boundary == GOL_BOUNDED, (int)(b->rule & 0x1FF), (int)(b->rule >> 9),
                                                b->stream));
        else
            GOL_HIP(gol::launch_bytes_step(b->cells(b->cur), b->cells(b->cur ^ 1), b->W, b->H,
                                           b->boundary == GOL_BOUNDED, b->stream));
        return GOL_OK;
    });
}

// the rule-generic streaming pass: passes of rule_stream_max_k generations (4; "rule_k": up to 8), then the binary
// remainder
int run_rule_stream(gol_board* b, int64_t gens) {
    const int cap = b->opt.rule_k ? b->opt.rule_k : gol::rule_stream_max_k(b->ilv);
    return ping_pong(b, &b->cur, gens,
                     [cap](int64_t left) { return (int64_t)gol::rule_stream_largest_k(std::min<int64_t>(left, cap)); },
                     [&](int64_t g) {
                         GOL_HIP(gol::launch_rule_stream(b->words(b->cur), b->words(b->cur ^ 1), b->W, b->H, b->pitch,
                                                         b->ilv, (int)g, b->boundary == GOL_BOUNDED, b->rule,
                                                         b->opt.rule_seg_rows, b->stream));
                         return GOL_OK;
                     });
}

// the multi-plane streaming pass of a Generations board: passes of gen_stream_max_k generations (gol_gen_plan.h;
// "rule_k" 4, 2, 1 force a depth), then the binary remainder; the decay planes ping-pong with the alive plane
int run_gen_stream(gol_board* b, int64_t gens) {
    if (b->opt.rule_k == 8)
        return fail(GOL_ERR_UNSUPPORTED, "rule_k 8: the multi-plane streaming pass of a Generations board runs 4, 2 or 1 "
                                         "generations per pass");
    const int cap = b->opt.rule_k ? b->opt.rule_k
                                  : gol::gen_stream_max_k(b->ilv, gol::gen_planes(b->nstates), b->boundary == GOL_BOUNDED);
    return ping_pong(b, &b->cur, gens, [cap](int64_t left) { return (int64_t)gol::gen_stream_largest_k(left, cap); },
                     [&](int64_t g) {
                         GOL_HIP(gol::launch_gen_stream(b->words(b->cur), b->words(b->cur ^ 1), b->dec_words(b->cur),
                                                        b->dec_words(b->cur ^ 1), b->W, b->H, b->pitch, b->ilv, (int)g,
                                                        b->boundary == GOL_BOUNDED, b->rule, b->nstates,
                                                        b->opt.rule_seg_rows, b->stream));
                         return GOL_OK;
                     });
}

// The two passes on a ragged byte board's scratch rows: packed once -- ceil(W / 32) words per row, a
// Generations board's decay planes behind the alive rows -- and kept there after the call (rag_state 1 / 4); the depths
// and the remainder chain are those of the packed boards' passes above.
int run_rule_ragged(gol_board* b, int64_t gens) {
    const int64_t nw = (b->W + 31) / 32;
    if (b->rag_state != 1) {
        GOL_RC(ensure_rag(b, nw * b->H));
        GOL_HIP(gol::launch_pack_ragged(b->cells(b->cur), b->rag[0], b->W, b->H, nw, b->stream));
        b->rag_cur = 0;
    }
    b->rag_state = 1;
    b->rag_pitch = nw;
    const int cap = b->opt.rule_k ? b->opt.rule_k : gol::rule_stream_max_k(1);
    return ping_pong(b, &b->rag_cur, gens,
                     [cap](int64_t left) { return (int64_t)gol::rule_stream_largest_k(std::min<int64_t>(left, cap)); },
                     [&](int64_t g) {
                         GOL_HIP(gol::launch_rule_stream_ragged(b->rag[b->rag_cur], b->rag[b->rag_cur ^ 1], b->W, b->H,
                                                                (int)g, b->boundary == GOL_BOUNDED, b->rule,
                                                                b->opt.rule_seg_rows, b->stream));
                         return GOL_OK;
                     });
}

int run_gen_ragged(gol_board* b, int64_t gens) {
    if (b->opt.rule_k == 8)
        return fail(GOL_ERR_UNSUPPORTED, "rule_k 8: the multi-plane streaming pass of a Generations board runs 4, 2 or 1 "
                                         "generations per pass");
    const int64_t nw = (b->W + 31) / 32, plane = nw * b->H;
    const int planes = gol::gen_planes(b->nstates);
    if (b->rag_state != 4) {
        GOL_RC(ensure_rag(b, plane * (1 + planes)));
        GOL_HIP(gol::launch_pack_ragged(b->cells(b->cur), b->rag[0], b->W, b->H, nw, b->stream));
        GOL_HIP(gol::launch_pack_ragged_decay(b->dec_cells(b->cur), b->rag[0] + plane, b->W, b->H, nw, planes, b->stream));
        b->rag_cur = 0;
    }
    b->rag_state = 4;
    b->rag_pitch = nw;
    const int cap = b->opt.rule_k ? b->opt.rule_k : gol::gen_stream_max_k(1, planes, b->boundary == GOL_BOUNDED);
    return ping_pong(b, &b->rag_cur, gens, [cap](int64_t left) { return (int64_t)gol::gen_stream_largest_k(left, cap); },
                     [&](int64_t g) {
                         uint32_t *src = b->rag[b->rag_cur], *dst = b->rag[b->rag_cur ^ 1];
                         GOL_HIP(gol::launch_gen_stream_ragged(src, dst, src + plane, dst + plane, b->W, b->H, (int)g,
                                                               b->boundary == GOL_BOUNDED, b->rule, b->nstates,
                                                               b->opt.rule_seg_rows, b->stream));
                         return GOL_OK;
                     });
}

// Generations of the next streaming pass of a packed board with `left` to go, and that pass
int stream_depth(const gol_board* b, int64_t left) {
    return gol::stream_largest_k(left, b->tblock, b->ilv, b->W / 32, b->boundary == GOL_BOUNDED);
}
int stream_pass(gol_board* b, int k) {
    gol::StreamArgs a = b->stream_args(0, b->H, k);
    GOL_HIP(gol::launch_stream_step(b->words(b->cur), b->words(b->cur ^ 1), a, k, b->boundary == GOL_BOUNDED,
                                    b->boundary == GOL_TORUS, b->stream));
    return GOL_OK;
}
int run_stream(gol_board* b, int64_t gens) {
    if (b->ilv == 4)  // the level-pipelined pass reports a timed-out ring wait in the board's error word
        GOL_RC(ensure_err_word(b));
    return ping_pong(b, &b->cur, gens, [&](int64_t left) { return (int64_t)stream_depth(b, left); },
                     [&](int64_t g) { return stream_pass(b, (int)g); });
}

// The scratch-row state (gol_board::rag_state) a pass leaves a ragged board in; every other pass needs the bytes.
int rag_state_of(Pass p) {
    if (p == gol::kPassRuleRagged) return 1;  // the streaming pass's rows under another kernel
    if (p == gol::kPassGenRagged) return 4;
    return p == Pass::StreamRagged ? 1 : (p == Pass::CoopRagged ? 2 : (p == Pass::Ring ? 3 : 0));
}

int step_impl(gol_board* b, int64_t gens) {
    if (gens <= 0) return GOL_OK;
    const gol::PassChoice c = gol::choose_pass(b, gens);
    b->last_pass = c.pass;
    if (b->rag_state != rag_state_of(c.pass)) GOL_RC(sync_bytes(b));
    if (c.pass == gol::kPassGenStream) return run_gen_stream(b, gens);
    if (c.pass == gol::kPassRuleRagged) return run_rule_ragged(b, gens);
    if (c.pass == gol::kPassGenRagged) return run_gen_ragged(b, gens);
    switch (c.pass) {
        case Pass::Multi: return b->multi->step(gens, &b->generation);
        case Pass::Wave: return run_wave(b, gens);
        case Pass::Lanes: return run_coop(b, gens, true);
        case Pass::Coop: return run_coop(b, gens, false);
        case Pass::CoopRagged: return run_coop_ragged(b, gens, c.rag_pitch);
        case Pass::Ring: return run_ring(b, gens);
        case Pass::StreamRagged: return run_stream_ragged(b, gens);
        case Pass::Resident: return run_resident(b, gens);
        case Pass::Bytes: return run_bytes(b, gens);
        case Pass::Stream: return run_stream(b, gens);
        case Pass::RuleStream: return run_rule_stream(b, gens);
        case Pass::None: break;
    }
    return GOL_OK;
}

}  // namespace

extern "C" {

int gol_step(gol_board* b, int64_t generations) {
    return with_board(b, [&] {
        if (generations < 0) return fail(GOL_ERR_INVALID, "negative generations");
        return step_impl(b, generations);
    });
}

int gol_pass_timing(gol_board* b, int n, double* interior_us, double* wait_us, double* edge_us) {
    return with_board(b, [&] {
        const int parts = b->multi ? b->multi->parts() : 1;
        if (n != parts || !interior_us || !wait_us || !edge_us)
            return fail(GOL_ERR_INVALID, "n must equal gol_num_parts and the arrays must be non-null");
        if (b->multi) return b->multi->timed_pass(interior_us, wait_us, edge_us, &b->generation);
        if (b->nstates > 2)
            return fail(GOL_ERR_UNSUPPORTED, "pass timing measures the B3/S23 streaming pass: this board runs a "
                                             "Generations rule (gol_set_generations_rule; gol_step_timed times any)");
        if (b->rule_family())
            return fail(GOL_ERR_UNSUPPORTED, "pass timing measures the B3/S23 streaming pass: this board runs another "
                                             "rule (gol_set_rule) or the rule family's passes (gol_step_timed times any)");
        if (!b->packed) return fail(GOL_ERR_UNSUPPORTED, "pass timing needs a bit-packed board");
        // a single board's timed pass is one streaming pass: boards whose gol_step takes another pass are refused, so
        // the figure always describes the pass the board runs.  The rows-on-lanes pass only replaces the cooperative
        // one on long calls: where a call of k generations would take it, a shorter call's pass decides.
        const int k = stream_depth(b, b->tblock);
        Pass p = gol::choose_pass(b, k).pass;
        if (p == Pass::Lanes) p = gol::choose_pass(b, 1).pass;
        if (p != Pass::Stream)
            return fail(GOL_ERR_UNSUPPORTED, "pass timing: this board's gol_step runs the single-wave, cooperative or "
                                             "LDS-resident pass, not the streaming pass the timing measures");
        if (b->ilv == 4) GOL_RC(ensure_err_word(b));
        gol::EventPair ev;
        GOL_RC(ev.create());
        GOL_HIP(hipEventRecord(ev.e0, b->stream));
        GOL_RC(stream_pass(b, k));
        GOL_HIP(hipEventRecord(ev.e1, b->stream));
        GOL_RC(ev.elapsed_us(&interior_us[0]));
        b->cur ^= 1;
        b->generation += k;
        wait_us[0] = 0;
        edge_us[0] = interior_us[0];
        return GOL_OK;
    });
}

int gol_step_timed(gol_board* b, int64_t generations, double* elapsed_us) {
    return with_board(b, [&] {
        if (!elapsed_us) return fail(GOL_ERR_INVALID, "null elapsed_us");
        if (generations < 0) return fail(GOL_ERR_INVALID, "negative generations");
        if (b->multi) {
            b->last_pass = Pass::Multi;
            return b->multi->step_timed(generations, &b->generation, elapsed_us);
        }
        gol::EventPair ev;
        GOL_RC(ev.create());
        GOL_HIP(hipEventRecord(ev.e0, b->stream));
        GOL_RC(step_impl(b, generations));
        GOL_HIP(hipEventRecord(ev.e1, b->stream));
        GOL_RC(ev.elapsed_us(elapsed_us));
        return check_valid(b);
    });
}

}  // extern "C"
