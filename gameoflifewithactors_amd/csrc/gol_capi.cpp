// gol_capi.cpp -- the C ABI (include/gol/gol.h): board handles, seeding, stepping, readback.
//
// This file is the native runtime around the kernels: it owns device memory, picks the kernel
// (bit-packed streaming step when width % 32 == 0, byte-per-cell step otherwise), splits a request
// for N generations into temporal-blocked passes, and maps every HIP failure to a GOL_ERR_* code with a
// thread-local message.  No C++ exception escapes an extern "C" function.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gol/gol.h"
#include "gol_debug.h"
#include "gol_debug.h"
#include "gol_internal.h"
#include "gol_multi.h"
#include "gol_view.h"

namespace {

thread_local std::string g_last_error;

// The test and A/B knobs of gol_debug.h (gol_debug_set_option), refused by gol_set_option with a pointer there.
// The names gol_debug_set_option / gol_debug_get_option take (csrc/gol_debug.h): ONE list, exported by
// gol_debug_option_names() so the Python side (_lib.DEBUG_OPTIONS) is checked against it
constexpr const char* kDebugOptions[] = {"coop_epoch", "coop_spin_limit", "coop_r", "resident_threads", "coop_launch",
                                         "lanes_launches"};
bool is_debug_option(const std::string& n) {
    for (const char* d : kDebugOptions)
        if (n == d) return true;
    return false;
}

// Every board call runs on the board's device whatever device the calling thread has current (staging
// buffers are allocated on the current device), and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define GOL_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(GOL_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// ---------------------------------------------------------------- .NET Framework System.Random
// Product restatement used by gol_seed_dotnet (GameOfLifeDriver.fs:10-11, GameofLife.fs:141-142,
// Script.fsx:25,27): Knuth subtractive generator, MSEED 161803398, 56-entry table, inext/inextp 0/21.
class DotNetRandom {
   public:
    explicit DotNetRandom(int32_t seed) {
        const int32_t mbig = 2147483647;
        int32_t sub = (seed == INT32_MIN) ? mbig : std::abs(seed);
        int32_t mj = 161803398 - sub, mk = 1;
        table_[55] = mj;
        for (int i = 1; i < 55; i++) {
            int ii = (21 * i) % 55;
            table_[ii] = mk;
            mk = (int32_t)((uint32_t)mj - (uint32_t)mk);
            if (mk < 0) mk += mbig;
            mj = table_[ii];
        }
        for (int k = 1; k < 5; k++)
            for (int i = 1; i < 56; i++) {
                table_[i] = (int32_t)((uint32_t)table_[i] - (uint32_t)table_[1 + (i + 30) % 55]);
                if (table_[i] < 0) table_[i] += mbig;
            }
    }
    int32_t Next() { return sample(); }
    int32_t Next(int32_t max_value) { return (int32_t)(sample() * (1.0 / 2147483647) * max_value); }

   private:
    int32_t sample() {
        if (++inext_ >= 56) inext_ = 1;
        if (++inextp_ >= 56) inextp_ = 1;
        int32_t r = (int32_t)((uint32_t)table_[inext_] - (uint32_t)table_[inextp_]);
        if (r == 2147483647) r--;
        if (r < 0) r += 2147483647;
        table_[inext_] = r;
        return r;
    }
    int32_t table_[56] = {0};
    int inext_ = 0, inextp_ = 21;
};

// ---------------------------------------------------------------- RLE (Life run-length encoding)
bool parse_rle(const char* p, std::vector<std::pair<int64_t, int64_t>>& out, std::string& err) {
    if (!p) {
        err = "null RLE";
        return false;
    }
    // skip '#' comment lines and the "x = .., y = .." header line
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
        if (*p == '#' || *p == 'x') {
            while (*p && *p != '\n') p++;
            continue;
        }
        break;
    }
    int64_t dx = 0, dy = 0, count = 0;
    for (; *p && *p != '!'; p++) {
        const char c = *p;
        if (c >= '0' && c <= '9') {
            count = count * 10 + (c - '0');
            if (count > (int64_t)1 << 40) {
                err = "RLE run length too large";
                return false;
            }
            continue;
        }
        if (c == ' ' || c == '\t' || c == '\r' || c == '\n') continue;
        const int64_t n = count ? count : 1;
        count = 0;
        if (c == '$') {
            dy += n;
            dx = 0;
        } else if (c == 'b' || c == '.') {
            dx += n;
        } else if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) {
            for (int64_t i = 0; i < n; i++) out.emplace_back(dx + i, dy);
            dx += n;
        } else {
            err = std::string("bad RLE character '") + c + "'";
            return false;
        }
    }
    return true;
}

// temporal-block depths accepted as a cap (gol_create's tblock_k); each layout supports a subset
bool valid_k(int k) {
    return k == 1 || k == 2 || k == 4 || k == 6 || k == 8 || k == 12 || k == 16 || k == 24 || k == 32;
}

// Interleave for a packed board of this width (gol_layout.h).  Measured on MI355X at 65536^2
// (profiles/r1/sweep_ilv.log, w12_sweep*.log): ilv 2 with K = 12 is the fastest configuration, ilv 4 needs 240 window
// VGPRs at K = 8 (2 waves/SIMD) and wastes 1/9 of its lanes on a 65536-wide row, ilv 1 pays 4x the
// funnel shifts.  gol_create_ex takes an explicit interleave (experiments).
int pick_ilv(int64_t width) {
    if (width % 64 == 0) return 2;
    return 1;
}

// Default generations per pass for a layout (measured on MI355X, DESIGN.md "Temporal block depth").
int default_tblock(int ilv) { return ilv == 4 ? 8 : (ilv == 2 ? 12 : 32); }

// Boards below this many cells are latency-bound, not throughput-bound: too few rows per wave to fill the
// device, so a deep pass is one long serial chain per wave.  They get narrow strips (ilv 1) and a shallow
// block (K = 8): 4096^2 8.8k vs 3.8k GCUPS at the large-board default (ilv 2, K = 12), 1024^2 554 vs 240,
// 256^2 bounded 21.7 vs 13.3 (profiles/r1/small_sweep.log).
constexpr int64_t kSmallBoardCells = (int64_t)1 << 25;
// Mid-size boards (up to 2^29 cells) run one level deeper at ilv 2: 16384^2 K = 16 56.1k vs K = 12 54.1k.
constexpr int64_t kMidBoardCells = (int64_t)1 << 29;
// LDS-resident pass (gol_resident.hip) cut-overs, measured on MI355X (profiles/r1/resident_small.log):
// packed 256^2 0.91 vs 1.47 us/generation on the streaming pass, 512x256 1.23 vs 1.47, but 512^2 1.87 vs
// 1.49.  Byte boards: off by default.  The ragged boards it could still take (the single-wave pass takes
// W <= 128 and H <= 256, the reference's 100^2 board included) ran slower on it than on the per-generation
// byte step in an interleaved A/B: 129x127 3.46 vs 3.10 us/generation, 200x100 3.65 vs 3.10, 181^2 6.26 vs
// 3.15, 255x257 10.7 vs 3.1; only 255x64 was level, 3.00 vs 3.12 (profiles/r2/byte_cut_ab.log).
// The board option "resident_max_cells" still forces it (tests).
constexpr int64_t kResidentMaxCells = (int64_t)1 << 17;
constexpr int64_t kResidentBytesMaxCells = 0;
constexpr int64_t kResidentMaxGensPerLaunch = (int64_t)1 << 16;
// Cooperative register-band pass (gol_coop.hip) for packed boards the single-wave pass does not take, up to this
// many cells and 8192 wide: 4096^2 0.81 vs 1.62 us/generation on the streaming pass, 2048^2 0.44 vs 1.48, 512^2
// 0.50 vs 1.49 (profiles/r2/ab_coop_xh_u.log), 8192 x 4096 1.76 vs 2.95, 8192^2 2.16 vs 4.25, 4096 x 8192 1.01
// vs 4.14 (coop_wide_u.log, coop_wide_s.log); below the LDS-resident cut-over too: 256^2 bounded 0.41 vs 0.92 on
// the LDS-resident pass, 512 x 256 0.50 vs 1.22 (cut_resident_q.log).  The board options "coop" (0 disables it:
// the LDS-resident and streaming passes then take these boards) and "coop_max_cells" move the cut-over.
constexpr int64_t kCoopMaxCells = (int64_t)1 << 26;
constexpr int kCoopFlagWords = 1024;            // bands of one launch at most (one per CU) ...
constexpr int kCoopErrWord = kCoopFlagWords - 1;  // ... and the error word
constexpr int64_t kCoopMaxGensPerLaunch = 32768;  // a launch's granule tags count its blocks in 16 bits

// The level-pipelined pass (gol_pipe.hip): boards (or strips) of at least this many cells whose rows
// hold at least one strip of blocks of 128 cells -- 62 stored on a torus, 64 on a bounded board -- get ilv 4 and its
// depth (bounded 65536^2 in the driver's window: 124.0-124.7k GCUPS against 120.9-121.7k for the streaming pass's
// ilv 2, K = 12, profiles/r6/bounded/)
constexpr int64_t kPipeMinCells = (int64_t)1 << 30;
constexpr int kPipeK = 32;
bool pipe_shape(int64_t width, int64_t rows, int boundary) {
    return width % 128 == 0 && width / 128 >= (boundary == GOL_TORUS ? 62 : 64) && width * rows >= kPipeMinCells;
}

// Layout and depth a new board gets when the caller leaves them at 0.  nparts: row strips (devices) of the board.
int board_ilv(int64_t width, int64_t height, int nparts, int boundary) {
    const int64_t cells = width * height;
    if (pipe_shape(width, height / nparts, boundary)) return 4;
    // single boards the cooperative pass takes: its interleave, so a block costs 2 funnel shifts instead of 2 per
    // word (a multi-GPU board never runs that pass: it keeps the streaming layout)
    const int m = width % 32 == 0 ? gol::coop_m(width / 32) : 0;
    if (nparts == 1 && m > 1 && cells > kResidentMaxCells && cells <= kCoopMaxCells) return m;
    return cells < kSmallBoardCells ? 1 : pick_ilv(width);
}

int board_tblock(int ilv, int64_t cells, int boundary) {
    // byte boards (ragged widths): the ragged streaming pass runs ilv 1 words, as small ilv-1 boards do; one level
    // deeper above 2^27 cells (torus, per generation, K = 16 / 24: 10001^2 3.6-3.8 / 4.4-4.6 us, 16383^2 7.7-8.2 /
    // 7.0-7.2, 23171^2 12.5-12.9 / 12.0-12.3, 32767^2 23.2-23.5 / 22.3-22.4, 65535^2 84.4-85.6 / 83.7-84.1;
    // profiles/r3/ragged_stream_k_b.log, ragged_stream_k_m.log)
    if (ilv == 0) return cells < kSmallBoardCells ? 8 : (cells < ((int64_t)1 << 27) ? 16 : 24);
    if (ilv == 1 && cells < kSmallBoardCells) return 8;
    // Mid-size boards run one level deeper.  Large bounded boards ran best at K = 16 in rounds 1-2 (the masked
    // variant); since round 3's staged passes K = 12 leads there as on the torus: the whole 10k-generation job at
    // 65536^2 127.5k vs 119.2k GCUPS (profiles/r3/bench_bounded_job_d.log).  Ghost-row strips (multi-GPU) keep
    // K = 12: over a whole job 114k vs 100k GCUPS for K = 16 (profiles/r1/strip_k_ab.log).
    if (ilv == 2 && cells < kMidBoardCells) return 16;
    if (ilv == 4 && cells >= kPipeMinCells) return kPipeK;
    return default_tblock(ilv);
}

}  // namespace

namespace gol {
int api_fail(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace gol

// Per-board path and tuning options (gol_set_option).  The library reads no environment variable: a stray one in
// the host process cannot change kernel paths.  Defaults are the measured ones.
struct BoardOptions {
    bool coop = true;                         // "coop": cooperative register-band pass for mid-size boards
    int coop_k = 0;                           // "coop_k": generations per hand-off (0 = min(tblock_k, 8))
    int64_t coop_max_cells = kCoopMaxCells;   // "coop_max_cells": largest board the cooperative pass takes
    int64_t resident_max_cells = -1;          // "resident_max_cells": LDS-resident cut-over (-1 = per layout)
    bool wave_resident = true;                // "wave_resident": single-wave pass for boards <= 128 x 256
    int32_t split = 0;                        // "split": streaming pair split, 1/65536 (0 = engine, < 0 = off)
    int32_t split2 = 0;                       // "split2": three-wave groups, the middle wave's share of the two
                                              // younger waves' rows, 1/65536 (0 = engine)
    int64_t seg_rows = 0;                     // "seg_rows": streaming rows per wave segment (0 = planned)
    int seam = 0;                             // "seam": torus seam strips (0 = where they apply, -1 = off)
    bool ragged_stream = true;                // "ragged_stream": ragged boards beyond the cooperative pass stream
                                              // packed words (0: the per-generation byte step)
    int ragged_ring = 1;                      // "ragged_ring": ragged boards stream as block rows (torus: ring rows on
                                              // the aligned kernel; bounded: column-masked block rows) in the aligned
                                              // layouts: 1 from kRingMinCells cells, 2 always, 0 never (ilv-1 rows,
                                              // bit-level row ends on a torus)
    int coop_r = 1;                           // "coop_r": cooperative pass, rows per wave at least
    int coop_poll_delay = -1;                 // "coop_poll_delay": s_sleep periods before a hand-off's first poll
                                              // (-1: 0 on the cooperative pass's rows of <= 2048 cells, else 8)
    int64_t coop_spin_limit = 0;              // "coop_spin_limit": polls before a hand-off wait gives up (0 = ~2 s)
    int resident_threads = 1024;              // "resident_threads": LDS-resident workgroup size (1024 or 256)
    int lanes = 2;                            // "lanes": rows-on-lanes band pass (gol_lanes.hip) in place of the
                                              // cooperative one, for calls of >= 2 * coop depth: 2 = where it
                                              // measured faster (use_lanes), 1 = wherever it applies, 0 = never
    int lanes_m = 0;                          // "lanes_m": its words per lane and half-row (0 = by width, 5, 9, 17)
    int32_t pipe_split = 0;                   // "pipe_split": level-pipelined pass (gol_pipe.hip), the oldest
                                              // pipeline's share of a pair, 1/65536 (0 = engine, < 0 = equal shares)
    int32_t pipe_split2 = 0;                  // "pipe_split2": its ratio after the second-oldest (0 = pipe_split)
    bool coop_launch = false;                 // "coop_launch": persistent passes by hipLaunchCooperativeKernel (1), or
                                              // hipLaunchKernel after the same residency check (0, the default:
                                              // gol_internal.h launch_persistent)
    bool view_stream = true;                  // "view_stream": wide-tile views on the streaming kernel (gol_view.hip);
                                              // 0 = every view on the per-pixel kernel
};

struct gol_board {
    std::mutex mu;
    BoardOptions opt;
    bool invalid = false;  // a cooperative hand-off timed out: readbacks fail until the board is overwritten
    bool invalid_pipe = false;  // ... or a ring wait of the level-pipelined pass (gol_pipe.hip)
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t W = 0, H = 0;
    int boundary = GOL_TORUS;
    int tblock = 16;
    bool tblock_set = false;  // tblock_k was given at creation (a cap), not the engine default
    bool packed = false;
    int ilv = 0;        // words per interleaved block (packed boards), 0 = byte board
    int64_t pitch = 0;  // words per row (packed)
    void* buf[2] = {nullptr, nullptr};
    int cur = 0;
    unsigned long long* acc = nullptr;  // device scratch accumulator
    unsigned* coop = nullptr;           // cooperative pass: per-band flags + error word (allocated on first use)
    uint32_t* coop_xch = nullptr;       // cooperative pass: hand-off granules (allocated on first use)
    int64_t coop_xch_words = 0;
    unsigned coop_epoch = 0;            // tag epoch of the last cooperative launch (1..65535)
    int64_t lanes_launches = 0;         // launches of the rows-on-lanes pass on this board (option "lanes_launches")
    uint32_t* rag[2] = {nullptr, nullptr};  // ragged byte boards on the cooperative pass: whole-word scratch rows
    int64_t rag_words = 0;                  // capacity of each rag buffer
    // Ragged byte boards between gol_step calls of the multi-generation passes keep their state in the scratch rows:
    // 0 = the bytes (cells(cur)) are current; 1 = rag[rag_cur] holds it in the streaming pass's rows (rag_pitch words),
    // 2 = in the cooperative pass's rows, 3 = in ring rows (gol_formats.hip, layout rag_ilv).  Every other access first
    // brings the bytes up to date (sync_bytes).
    int rag_state = 0;
    int rag_cur = 0;
    int64_t rag_pitch = 0;
    int rag_ilv = 1;
    int ring_age = 0;  // ring rows: generations since the copies were last exact (errors reach ring_age cells in)
    int64_t generation = 0;
    gol::MultiBoard* multi = nullptr;  // num_gpus > 1: row strips over several devices (gol_multi.h)

    size_t bytes() const { return packed ? (size_t)(pitch * H) * 4 : (size_t)(W * H); }
    uint32_t* words(int i) { return static_cast<uint32_t*>(buf[i]); }
    uint8_t* cells(int i) { return static_cast<uint8_t*>(buf[i]); }

    gol::StreamArgs stream_args(int64_t out_begin, int64_t out_end, int k) const {
        gol::StreamArgs a{};
        a.words = W / 32;
        a.pitch = pitch;
        a.rows = H;
        a.ghost = 0;
        a.y0 = 0;
        a.height = H;
        a.out_begin = out_begin;
        a.out_end = out_end;
        a.seg = 0;
        a.ilv = ilv;
        a.split_opt = opt.split;
        a.split2_opt = opt.split2;
        a.seg_opt = opt.seg_rows;
        a.seam_opt = opt.seam;
        a.pipe_split_opt = opt.pipe_split;
        a.pipe_split2_opt = opt.pipe_split2;
        a.pipe_err = coop ? reinterpret_cast<int*>(coop + kCoopErrWord) : nullptr;
        return a;
    }
};

namespace {

// The entry points switch to the board's device through DeviceGuard (constructed after this check), which
// restores the caller's current device on return.
int check_board(gol_board* b) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    return GOL_OK;
}

// After the board's stream has drained: a cooperative pass whose hand-off wait timed out left a wrong board.  Its
// error word is read (and cleared) here, after every synchronisation a caller can observe -- gol_synchronize and
// every readback -- and the board stays invalid until it is overwritten (set_cells, load, seed, clear).
int check_valid(gol_board* b) {
    if (b->coop) {
        int err = 0;
        GOL_HIP(hipMemcpyAsync(&err, b->coop + kCoopErrWord, sizeof(int), hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        if (err) {
            b->invalid = true;
            b->invalid_pipe = (err & 2) != 0;  // gol_pipe.hip sets bit 1, the persistent passes 1
            GOL_HIP(hipMemsetAsync(b->coop + kCoopErrWord, 0, sizeof(unsigned), b->stream));
            GOL_HIP(hipStreamSynchronize(b->stream));
        }
    }
    if (b->invalid && b->invalid_pipe)
        return fail(GOL_ERR_HIP, "level-pipelined pass: a ring wait between the waves of one workgroup timed out (a "
                                 "library defect: every wave it waits on is resident); creating the board with ilv 2 "
                                 "avoids the pass; the board is invalid until it is overwritten (set_cells, load, "
                                 "seed, clear)");
    if (b->invalid)
        return fail(GOL_ERR_HIP, "persistent pass: a band hand-off timed out -- the pass could not get every CU at "
                                 "once (another process or stream holds the device); board option \"coop\" 0 "
                                 "avoids the persistent passes; the board is invalid until it is overwritten "
                                 "(set_cells, load, seed, clear)");
    return GOL_OK;
}

int sync(gol_board* b) {
    if (b->multi) return b->multi->synchronize();
    GOL_HIP(hipStreamSynchronize(b->stream));
    return check_valid(b);
}

// The board's cells were replaced as a whole: a timed-out hand-off no longer matters, and a ragged board's scratch
// rows no longer hold its state.  The stream is drained first (the overwrite was queued behind any earlier pass),
// then the cooperative error word is cleared WITHOUT marking the board invalid: an error a timed-out pass left
// there, with no readback or gol_synchronize after it, must not fail the overwrite that replaces its result
// (tests/test_gpu_coop.py::test_coop_timeout_then_overwrite_without_readback).
int overwritten(gol_board* b) {
    if (b->multi) {
        b->invalid = false;
        b->rag_state = 0;
        return b->multi->synchronize();
    }
    GOL_HIP(hipStreamSynchronize(b->stream));
    if (b->coop) {
        GOL_HIP(hipMemsetAsync(b->coop + kCoopErrWord, 0, sizeof(unsigned), b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
    }
    b->invalid = false;
    b->rag_state = 0;
    return GOL_OK;
}

// A ragged byte board whose state the multi-generation passes left in the scratch rows (rag_state): unpack it into
// the bytes, on the board's stream, before anything reads or modifies them.
int sync_bytes(gol_board* b) {
    if (!b->rag_state) return GOL_OK;
    if (b->rag_state == 3)
        GOL_HIP(gol::launch_unpack_ring(b->rag[b->rag_cur], b->cells(b->cur), b->W, b->H, b->rag_ilv,
                                        b->boundary == GOL_TORUS, b->stream));
    else
        GOL_HIP(gol::launch_unpack_ragged(b->rag[b->rag_cur], b->cells(b->cur), b->W, b->H, b->rag_pitch, b->stream));
    b->rag_state = 0;
    return GOL_OK;
}

int set_cells_impl(gol_board* b, const uint8_t* host) {
    if (b->multi) return b->multi->set_cells(host);
    const size_t n = (size_t)(b->W * b->H);
    if (!b->packed) {
        GOL_HIP(hipMemcpyAsync(b->cells(b->cur), host, n, hipMemcpyHostToDevice, b->stream));
        return overwritten(b);
    }
    uint8_t* staging = nullptr;
    hipError_t e = hipMalloc(&staging, n);
    if (e != hipSuccess) return fail(GOL_ERR_OOM, std::string("hipMalloc staging: ") + hipGetErrorString(e));
    int rc = GOL_OK;
    do {
        e = hipMemcpyAsync(staging, host, n, hipMemcpyHostToDevice, b->stream);
        if (e != hipSuccess) break;
        e = gol::launch_pack(staging, b->words(b->cur), b->W, b->H, b->pitch, 0, b->ilv, b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    if (e != hipSuccess) rc = fail(GOL_ERR_HIP, std::string("set_cells: ") + hipGetErrorString(e));
    (void)hipFree(staging);
    return rc == GOL_OK ? overwritten(b) : rc;
}

int readback_impl(gol_board* b, uint8_t* host, int64_t stride, uint8_t value) {
    if (b->multi) return b->multi->readback(host, stride, value);
    if (int rc = sync_bytes(b)) return rc;
    const size_t n = (size_t)(stride * b->H);
    uint8_t* staging = nullptr;
    hipError_t e = hipMalloc(&staging, n);
    if (e != hipSuccess) return fail(GOL_ERR_OOM, std::string("hipMalloc staging: ") + hipGetErrorString(e));
    int rc = GOL_OK;
    do {
        if (stride != b->W) {
            e = hipMemsetAsync(staging, 0, n, b->stream);
            if (e != hipSuccess) break;
        }
        if (b->packed)
            e = gol::launch_unpack(b->words(b->cur), staging, b->W, b->H, b->pitch, 0, stride, value, b->ilv,
                                   b->stream);
        else
            e = gol::launch_bytes_render(b->cells(b->cur), staging, b->W, b->H, stride, value, b->stream);
        if (e != hipSuccess) break;
        e = hipMemcpyAsync(host, staging, n, hipMemcpyDeviceToHost, b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    if (e != hipSuccess) rc = fail(GOL_ERR_HIP, std::string("readback: ") + hipGetErrorString(e));
    (void)hipFree(staging);
    return rc == GOL_OK ? check_valid(b) : rc;
}

int reduce_impl(gol_board* b, bool hash, uint64_t* out) {
    if (b->multi) return b->multi->reduce(hash, out);
    if (int rc = sync_bytes(b)) return rc;
    GOL_HIP(hipMemsetAsync(b->acc, 0, sizeof(unsigned long long), b->stream));
    if (b->packed) {
        if (hash)
            GOL_HIP(gol::launch_hash_packed(b->words(b->cur), b->W, b->H, b->pitch, 0, 0, b->ilv, b->acc, b->stream));
        else
            GOL_HIP(gol::launch_popcount_packed(b->words(b->cur), b->W / 32, b->H, b->pitch, 0, b->acc, b->stream));
    } else {
        if (hash)
            GOL_HIP(gol::launch_hash_bytes(b->cells(b->cur), b->W, b->H, b->acc, b->stream));
        else
            GOL_HIP(gol::launch_popcount_bytes(b->cells(b->cur), b->W * b->H, b->acc, b->stream));
    }
    unsigned long long v = 0;
    GOL_HIP(hipMemcpyAsync(&v, b->acc, sizeof(v), hipMemcpyDeviceToHost, b->stream));
    GOL_HIP(hipStreamSynchronize(b->stream));
    if (int rc = check_valid(b)) return rc;
    *out = hash ? gol_hash_finalize(v, b->W, b->H) : (uint64_t)v;
    return GOL_OK;
}

// Boards up to this many cells run every gol_step call as ONE launch of the LDS-resident kernel
// (gol_resident.hip) when the layout fits it: whole board in one workgroup's LDS, one barrier per
// generation.  The board option "resident_max_cells" overrides (0 disables; tests/test_gpu_resident.py).
int64_t resident_max_cells(const gol_board* b) {
    if (b->opt.resident_max_cells >= 0) return b->opt.resident_max_cells;
    return b->packed ? kResidentMaxCells : kResidentBytesMaxCells;
}

// Boards small enough for one wavefront's registers (gol_wave.hip: W <= 128, H <= 256) run every gol_step call
// as one single-wave launch (board option "wave_resident" = 0 disables it).
bool use_wave_resident(const gol_board* b) {
    if (!b->opt.wave_resident) return false;
    return gol::wave_resident_rpl(b->W, b->H) > 0 && (!b->packed || b->ilv == 1);
}

// Generations per hand-off of the cooperative pass: the board's "coop_k" option if set, else its temporal-block
// cap, at most gol::kCoopDefaultK.
int coop_depth(const gol_board* b) {
    if (b->opt.coop_k > 0) return b->opt.coop_k;
    return b->tblock < gol::kCoopDefaultK ? b->tblock : gol::kCoopDefaultK;
}

// The rows-on-lanes band pass (gol_lanes.hip) on a packed single board, for a call of `gens` generations: the boards
// the cooperative pass would take whose width splits into windows (64 (m - 1) columns each), calls of at least two
// hand-off blocks (the pass stages the board through LDS at both ends of a launch).
// By default (option "lanes" 2) it takes the sizes where it measured faster than the cooperative pass: rows of <= 1024
// cells (profiles/r4/lanes_ab_j.log, us/generation, lanes vs cooperative: 256^2 0.35 vs 0.49, 512^2 0.37 vs 0.49, 1024 x
// 2048 0.41 vs 0.51).  Round 4 also gave it 8192-wide boards up to 4096 rows (m = 9: 8192 x 2048 1.08 vs 1.55); round
// 5's 16-byte granules took the cooperative pass there to 0.88-0.98 / 1.01-1.09 against 1.10 / 1.18 for the lanes
// (profiles/r5/coop_delay_ab_m.log, coop_errword_ab_l.log), so 2048- to 8192-wide boards are the cooperative pass's.
bool lanes_by_size(int64_t W, int64_t H) {
    (void)H;
    return W <= 1024;
}
// Its hand-off depth: the "coop_k" option if set, else up to 10 on rows of <= 1024 cells (the deepest a 32-row
// window holds beside a band of >= k rows; there the pass is hand-off bound: 256^2 bounded 0.32 vs 0.36 us/generation
// at k = 8, 512^2 0.33 vs 0.37, 1024 x 2048 0.36 vs 0.41, profiles/r4/lanes_k_o.log), else the cooperative depth.
int lanes_depth(const gol_board* b) {
    if (b->opt.coop_k > 0) return b->opt.coop_k;
    if (b->W > 1024) return coop_depth(b);
    return b->tblock_set && b->tblock < 10 ? b->tblock : 10;
}
bool use_lanes(const gol_board* b, int64_t gens) {
    if (!b->opt.lanes || !b->opt.coop || !b->packed || b->multi) return false;
    if (b->opt.lanes == 2 && !lanes_by_size(b->W, b->H)) return false;
    // every band resident at once: a tall narrow board plans more bands than the device holds
    return gens >= 2 * lanes_depth(b) && b->W * b->H <= b->opt.coop_max_cells &&
           gol::lanes_fits(b->W, b->H, lanes_depth(b), b->opt.lanes_m, b->ilv, b->boundary == GOL_BOUNDED);
}

bool use_coop(const gol_board* b) {
    if (!b->opt.coop || !b->packed) return false;
    const int cm = gol::coop_m(b->W / 32);
    int nwg = 0, B = 0, R = 0;
    return (b->ilv == 1 || b->ilv == cm) && b->W * b->H <= b->opt.coop_max_cells &&
           gol::coop_plan(b->W, b->H, coop_depth(b), &nwg, &B, &R, b->opt.coop_r) && nwg < kCoopFlagWords;
}

// Words per lane of the cooperative pass for a ragged row of nw words (rows padded to a multiple of it).
int coop_m_ragged(int64_t nw) { return nw <= 64 ? 1 : (nw <= 128 ? 2 : (nw <= 256 ? 4 : 0)); }

// Ragged byte boards (width not a multiple of 32) the single-wave pass does not take run on the cooperative pass
// through whole-word scratch rows when a call has at least this many generations: the per-generation byte step
// costs ~3.1 us per generation (profiles/r2/byte_cut_ab.log), the pack / unpack launches around the pass a few
// generations' worth.
constexpr int64_t kCoopRaggedMinGens = 16;
bool use_coop_ragged(const gol_board* b, int64_t* pitch) {
    if (!b->opt.coop || b->packed || b->W % 32 == 0) return false;
    const int64_t nw = (b->W + 31) / 32;
    const int cm = coop_m_ragged(nw);
    if (!cm || b->W * b->H > b->opt.coop_max_cells) return false;
    const int64_t nwp = (nw + cm - 1) / cm * cm;
    int nwg = 0, B = 0, R = 0;
    if (!gol::coop_plan(nwp * 32, b->H, coop_depth(b), &nwg, &B, &R, b->opt.coop_r) || nwg >= kCoopFlagWords)
        return false;
    *pitch = nwp;
    return true;
}

// The board's error word (b->coop[kCoopErrWord]): the persistent passes' timed-out hand-offs and the level-pipelined
// pass's timed-out ring waits (check_valid)
int ensure_err_word(gol_board* b) {
    if (!b->coop) {
        GOL_HIP(hipMalloc(&b->coop, kCoopFlagWords * sizeof(unsigned)));
        GOL_HIP(hipMemsetAsync(b->coop, 0, kCoopFlagWords * sizeof(unsigned), b->stream));
    }
    return GOL_OK;
}

// `gens` generations of the cooperative pass on packed rows of W cells (`pitch` words, layout `ilv`; ragged_w > 0:
// scratch rows of a ragged board of that width), ping-ponging between bufs[*cur] and bufs[*cur ^ 1]; *cur ends on
// the result.  One launch per kCoopMaxGensPerLaunch generations.
int coop_steps(gol_board* b, int64_t W, int64_t pitch, int ilv, int64_t ragged_w, uint32_t* const bufs[2], int* cur,
               int64_t gens, bool lanes = false) {
    if (int rc = ensure_err_word(b)) return rc;
    int nwg = 0, B = 0, R = 0;
    const int k = lanes ? lanes_depth(b) : coop_depth(b);
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
    while (gens > 0) {
        const int64_t g = gens < kCoopMaxGensPerLaunch ? gens : kCoopMaxGensPerLaunch;
        if (++b->coop_epoch > 0xffff) {  // tags of an earlier epoch could match again: clear the granules
            GOL_HIP(hipMemsetAsync(b->coop_xch, 0, (size_t)b->coop_xch_words * sizeof(uint32_t), b->stream));
            b->coop_epoch = 1;
        }
        if (lanes) ++b->lanes_launches;
        if (lanes)
            GOL_HIP(gol::launch_lanes_pass(bufs[*cur], bufs[*cur ^ 1], W, b->H, pitch, ilv, k, g,
                                           b->boundary == GOL_BOUNDED, b->coop_epoch,
                                           reinterpret_cast<int*>(b->coop + kCoopErrWord), b->coop_xch,
                                           b->coop_xch_words, b->stream, b->opt.lanes_m, tune));
        else
            GOL_HIP(gol::launch_coop_pass(bufs[*cur], bufs[*cur ^ 1], W, b->H, pitch, ilv, k, g,
                                          b->boundary == GOL_BOUNDED, b->coop_epoch,
                                          reinterpret_cast<int*>(b->coop + kCoopErrWord), b->coop_xch,
                                          b->coop_xch_words, b->stream, ragged_w, tune));
        *cur ^= 1;
        b->generation += g;
        gens -= g;
    }
    return GOL_OK;
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

// Ragged byte boards the cooperative pass does not take (wider than 8192 cells or above 2^26 cells) run the
// streaming pass on whole-word scratch rows -- ceil(W / 32) words, the last one partial, the row end closed at bit
// level (gol_step.hip kRagged; bounded: the column-masked variant) -- packed once per gol_step call of at least this
// many generations; shorter calls take the per-generation byte step.
constexpr int64_t kStreamRaggedMinGens = 4;
bool use_stream_ragged(const gol_board* b) {
    if (b->packed || b->W % 32 == 0 || !b->opt.ragged_stream) return false;
    return (b->W + 31) / 32 >= 64;  // rows of at least one wave strip (the strip geometry's assumption)
}

// Ragged boards on the streaming pass run as block rows (gol_formats.hip) in the aligned layouts.  Torus: ring rows
// of ring_pitch(W) words, the board's cells at positions 64 .. 64 + W - 1 and copies of its ends around them, stepped
// by the ALIGNED torus kernel (seam strips, interleaved blocks: the headline kernel's instruction stream) with the two
// copies rewritten after every pass.  Bounded: rows of ceil(W / 64) blocks, the last one partial, on edge-fill strips
// that AND per-word column masks at every level (gol_step.hip NARROW = 2).  Layout and depth follow the aligned rules
// for a board of that many cells (board_ilv / board_tblock): ilv 2 from 2^25 cells, K = 16 below 2^29, 12 above.
// Block rows beat the ilv-1 rows from about 2^27.6 cells (profiles/r4/ragged_ab_b.log, us/generation, torus /
// bounded): 65535^2 41-43 vs 60 / 44-47 vs 52-54, 16383^2 5.2 vs 6.0 / 5.7 vs 5.6; below they lose: 8193 x 20000 5.0
// vs 4.7 / 4.9 vs 4.5, 10001^2 4.7 vs 3.6 / 4.6 vs 3.4.  Option "ragged_ring": 1 = by this size, 2 = always, 0 = never.
constexpr int64_t kRingMinCells = (int64_t)3 << 26;
bool ring_by_size(int64_t W, int64_t H) { return W * H >= kRingMinCells; }
bool use_ring(const gol_board* b) {
    return b->opt.ragged_ring == 2 || (b->opt.ragged_ring == 1 && ring_by_size(b->W, b->H));
}
constexpr int kRingCopy = 64;  // cells copied at each end of a ring row (gol_formats.hip kRingPad; the suffix has >= 64)
int64_t ring_cells(int64_t W, int64_t H, int boundary) { return gol::ring_pitch(W, boundary == GOL_TORUS) * 32 * H; }
int ring_ilv(const gol_board* b) { return ring_cells(b->W, b->H, b->boundary) < kSmallBoardCells ? 1 : 2; }

int step_impl(gol_board* b, int64_t gens) {
    if (b->multi) return b->multi->step(gens, &b->generation);
    if (gens <= 0) return GOL_OK;
    // the pass this call takes on a ragged byte board: 2 = cooperative, 1 = streaming (both on whole-word scratch rows
    // that keep the state after the call), 0 = a byte pass (the bytes must be current)
    int64_t rag_pitch = 0;
    const bool wave = use_wave_resident(b);
    const int rag_next = wave ? 0
                              : (gens >= kCoopRaggedMinGens && use_coop_ragged(b, &rag_pitch)
                                     ? 2
                                     : (gens >= kStreamRaggedMinGens && use_stream_ragged(b) ? (use_ring(b) ? 3 : 1) : 0));
    if (b->rag_state != rag_next)
        if (int rc = sync_bytes(b)) return rc;
    if (wave) {
        while (gens > 0) {
            const int64_t g = gens < kResidentMaxGensPerLaunch ? gens : kResidentMaxGensPerLaunch;
            GOL_HIP(gol::launch_wave_resident(b->buf[b->cur], b->buf[b->cur ^ 1], b->W, b->H, b->pitch, g,
                                              b->boundary == GOL_BOUNDED, !b->packed, b->stream));
            b->cur ^= 1;
            b->generation += g;
            gens -= g;
        }
        return GOL_OK;
    }
    if (use_lanes(b, gens)) {
        uint32_t* bufs[2] = {b->words(0), b->words(1)};
        return coop_steps(b, b->W, b->pitch, b->ilv, 0, bufs, &b->cur, gens, true);
    }
    if (use_coop(b)) {
        uint32_t* bufs[2] = {b->words(0), b->words(1)};
        return coop_steps(b, b->W, b->pitch, b->ilv, 0, bufs, &b->cur, gens);
    }
    if (rag_next == 2) {
        // the ragged byte board as whole words in scratch rows (packed once, kept there after the call), the pass
        if (b->rag_state != 2) {
            if (int rc = ensure_rag(b, rag_pitch * b->H)) return rc;
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
    if (rag_next == 3) {
        // the ragged board as block rows (packed once, kept there after the call), the aligned streaming kernel
        const bool torus = b->boundary == GOL_TORUS;
        const int64_t pitch = gol::ring_pitch(b->W, torus);
        const int ilv = ring_ilv(b);
        if (b->rag_state != 3) {
            if (int rc = ensure_rag(b, pitch * b->H)) return rc;
            GOL_HIP(gol::launch_pack_ring(b->cells(b->cur), b->rag[0], b->W, b->H, ilv, torus, b->stream));
            b->rag_cur = 0;
            b->ring_age = 0;
        }
        b->rag_state = 3;
        b->rag_pitch = pitch;
        b->rag_ilv = ilv;
        while (gens > 0) {
            const int k = gol::stream_largest_k(gens, b->tblock, ilv);
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
            b->rag_cur ^= 1;
            b->generation += k;
            gens -= k;
        }
        return GOL_OK;
    }
    if (rag_next == 1) {
        // the ragged byte board as whole words in scratch rows (packed once, kept there after the call), streaming
        const int64_t nw = (b->W + 31) / 32;
        if (b->rag_state != 1) {
            if (int rc = ensure_rag(b, nw * b->H)) return rc;
            GOL_HIP(gol::launch_pack_ragged(b->cells(b->cur), b->rag[0], b->W, b->H, nw, b->stream));
            b->rag_cur = 0;
        }
        b->rag_state = 1;
        b->rag_pitch = nw;
        // a ragged board's default depth is the block rows' (create_impl); this M = 1 path keeps its own
        const int cap = b->tblock_set ? b->tblock : board_tblock(0, b->W * b->H, b->boundary);
        while (gens > 0) {
            const int k = gol::stream_largest_k(gens, cap, 1);
            gol::StreamArgs a = b->stream_args(0, b->H, k);
            a.words = nw;
            a.pitch = nw;
            a.ilv = 1;
            a.rag_bits = (int32_t)(b->W % 32);
            a.rag_w = b->boundary == GOL_BOUNDED ? b->W : 0;
            GOL_HIP(gol::launch_stream_step(b->rag[b->rag_cur], b->rag[b->rag_cur ^ 1], a, k, b->boundary == GOL_BOUNDED,
                                            b->boundary == GOL_TORUS, b->stream));
            b->rag_cur ^= 1;
            b->generation += k;
            gens -= k;
        }
        return GOL_OK;
    }
    if (b->W * b->H <= resident_max_cells(b) &&
        (b->packed ? b->ilv == 1 && gol::resident_packed_fits(b->W, b->H) : gol::resident_bytes_fits(b->W, b->H))) {
        const bool bounded = b->boundary == GOL_BOUNDED;
        while (gens > 0) {
            // one launch per 2^16 generations (a few tens of ms): a long gol_step stays interruptible by
            // readbacks and other work on the board's stream
            const int64_t g = gens < kResidentMaxGensPerLaunch ? gens : kResidentMaxGensPerLaunch;
            if (b->packed)
                GOL_HIP(gol::launch_resident_packed(b->words(b->cur), b->words(b->cur ^ 1), b->W, b->H, b->pitch, g,
                                                    bounded, b->stream, b->opt.resident_threads));
            else
                GOL_HIP(gol::launch_resident_bytes(b->cells(b->cur), b->cells(b->cur ^ 1), b->W, b->H, g, bounded,
                                                   b->stream, b->opt.resident_threads));
            b->cur ^= 1;
            b->generation += g;
            gens -= g;
        }
        return GOL_OK;
    }
    if (!b->packed) {
        for (int64_t g = 0; g < gens; g++) {
            GOL_HIP(gol::launch_bytes_step(b->cells(b->cur), b->cells(b->cur ^ 1), b->W, b->H,
                                           b->boundary == GOL_BOUNDED, b->stream));
            b->cur ^= 1;
            b->generation++;
        }
        return GOL_OK;
    }
    if (b->ilv == 4)  // the level-pipelined pass reports a timed-out ring wait in the board's error word
        if (int rc = ensure_err_word(b)) return rc;
    while (gens > 0) {
        const int k = gol::stream_largest_k(gens, b->tblock, b->ilv, b->W / 32, b->boundary == GOL_BOUNDED);
        gol::StreamArgs a = b->stream_args(0, b->H, k);
        GOL_HIP(gol::launch_stream_step(b->words(b->cur), b->words(b->cur ^ 1), a, k, b->boundary == GOL_BOUNDED,
                                        b->boundary == GOL_TORUS, b->stream));
        b->cur ^= 1;
        b->generation += k;
        gens -= k;
    }
    return GOL_OK;
}

int place_points(gol_board* b, const std::vector<int64_t>& xy) {
    const int64_t n = (int64_t)xy.size() / 2;
    if (n == 0) return GOL_OK;
    if (b->multi) return b->multi->place_points(xy);
    if (int rc = sync_bytes(b)) return rc;
    int64_t* d = nullptr;
    hipError_t e = hipMalloc(&d, xy.size() * sizeof(int64_t));
    if (e != hipSuccess) return fail(GOL_ERR_OOM, "hipMalloc points");
    int rc = GOL_OK;
    do {
        e = hipMemcpyAsync(d, xy.data(), xy.size() * sizeof(int64_t), hipMemcpyHostToDevice, b->stream);
        if (e != hipSuccess) break;
        e = gol::launch_set_points(b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->pitch, d, n, b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    if (e != hipSuccess) rc = fail(GOL_ERR_HIP, std::string("place_points: ") + hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}

void free_board(gol_board* b) {
    delete b->multi;
    for (auto& p : b->buf)
        if (p) (void)hipFree(p);
    if (b->acc) (void)hipFree(b->acc);
    if (b->coop) (void)hipFree(b->coop);
    if (b->coop_xch) (void)hipFree(b->coop_xch);
    for (uint32_t* r : b->rag)
        if (r) (void)hipFree(r);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int check_strip(const gol_strip* s) {
    if (!s) return fail(GOL_ERR_INVALID, "null strip");
    if (s->width < 32 || s->width % 32) return fail(GOL_ERR_INVALID, "strip width must be a positive multiple of 32");
    if (s->height < 3 || s->rows < 1 || s->y0 < 0 || s->y0 + s->rows > s->height)
        return fail(GOL_ERR_INVALID, "strip rows outside the board");
    if (s->pitch < s->width / 32) return fail(GOL_ERR_INVALID, "strip pitch smaller than the row");
    if (s->ghost < 0) return fail(GOL_ERR_INVALID, "negative ghost");
    if (s->boundary != GOL_TORUS && s->boundary != GOL_BOUNDED) return fail(GOL_ERR_INVALID, "bad boundary");
    if (s->ilv != 1 && s->ilv != 2 && s->ilv != 4) return fail(GOL_ERR_INVALID, "ilv must be 1, 2 or 4");
    if (s->width % (32 * s->ilv) || s->pitch % s->ilv)
        return fail(GOL_ERR_INVALID, "width must be a multiple of 32*ilv and pitch a multiple of ilv");
    if (s->wrap_rows && (s->ghost != 0 || s->rows != s->height || s->y0 != 0))
        return fail(GOL_ERR_INVALID, "wrap_rows requires the whole board in one strip with ghost = 0");
    return GOL_OK;
}

// A view of a width x height board (include/gol/gol.h gol_view): checked on the host, before any device work.
int check_view(const gol_view* v, int64_t width, int64_t height, int boundary) {
    if (!v) return fail(GOL_ERR_INVALID, "null view");
    if (v->scale < 1 || v->scale > gol::kViewMaxScale) return fail(GOL_ERR_INVALID, "view scale must be 1..32768");
    if (v->out_w < 1 || v->out_h < 1 || v->out_w > gol::kViewMaxPixels || v->out_h > gol::kViewMaxPixels ||
        v->out_w * v->out_h > gol::kViewMaxPixels)
        return fail(GOL_ERR_INVALID, "view needs out_w, out_h >= 1 and out_w * out_h <= 2^26");
    if (boundary == GOL_TORUS) {
        if (v->x < 0 || v->x >= width || v->y < 0 || v->y >= height)
            return fail(GOL_ERR_INVALID, "torus view: the origin must lie on the board");
        if (v->scale * v->out_w > width || v->scale * v->out_h > height)
            return fail(GOL_ERR_INVALID, "torus view: scale * out_w / out_h exceeds the board (cells would count twice)");
    } else {
        const int64_t lim = (int64_t)1 << 31;
        if (v->x < -lim || v->x > lim || v->y < -lim || v->y > lim)
            return fail(GOL_ERR_INVALID, "bounded view: the origin must lie in [-2^31, 2^31]");
    }
    return GOL_OK;
}

// k = 16 / 32 at ilv 4 is the level-pipelined pass (gol_pipe.hip): torus strips with a full strip of blocks per row
int check_pipe_strip(const gol_strip* s, int k) {
    if (s->ilv == 4 && gol::pipe_supported(k) &&
        !gol::pipe_applies(s->width / 32, 4, k, s->boundary == GOL_BOUNDED, 0))
        return fail(GOL_ERR_INVALID, "k = 16 / 32 at ilv 4 is the level-pipelined pass: strips at least 7936 cells wide "
                                     "(torus) or 8192 (bounded)");
    return GOL_OK;
}

// StreamArgs of a strip pass (gol_strip_step / gol_strip_plan and the multi board's launches)
gol::StreamArgs strip_args(const gol_strip* s, int64_t out_begin, int64_t out_end, int32_t split_opt, int64_t seg_opt,
                           int32_t seam_opt, int32_t split2_opt = 0) {
    gol::StreamArgs a{};
    a.words = s->width / 32;
    a.pitch = s->pitch;
    a.rows = s->rows;
    a.ghost = s->ghost;
    a.y0 = s->y0;
    a.height = s->height;
    a.out_begin = out_begin;
    a.out_end = out_end;
    a.seg = 0;
    a.ilv = s->ilv;
    a.spare = s->spare_waves > 0 ? s->spare_waves : 0;
    a.split_opt = split_opt;
    a.seg_opt = seg_opt;
    a.seam_opt = seam_opt;
    a.split2_opt = split2_opt;
    return a;
}

}  // namespace

namespace gol {

int strip_plan_opts(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t* waves, int64_t* seg_rows,
                    int32_t split_opt, int64_t seg_opt, int32_t seam_opt, int32_t split2_opt) {
    if (int rc = check_strip(s)) return rc;
    if (!gol::stream_supported(k, s->ilv)) return fail(GOL_ERR_INVALID, "k not supported for this ilv");
    if (int rc = check_pipe_strip(s, k)) return rc;
    if (out_begin < 0 || out_end > s->rows || out_begin > out_end) return fail(GOL_ERR_INVALID, "bad output rows");
    gol::StreamArgs a = strip_args(s, out_begin, out_end, split_opt, seg_opt, seam_opt, split2_opt);
    if (s->ilv == 4 && gol::pipe_supported(k)) {  // the level-pipelined pass: 16-wave workgroups
        gol::PipeArgs p = gol::pipe_args(a, s->boundary == GOL_BOUNDED);
        gol::plan_pipe(p, k, s->wrap_rows != 0, p.spare_waves);
        if (seg_rows) *seg_rows = p.grows;
        if (waves) *waves = gol::pipe_grid(p) * 16;
        return GOL_OK;
    }
    gol::plan_stream(a, k, s->boundary == GOL_BOUNDED, s->wrap_rows != 0);
    if (seg_rows) *seg_rows = a.seg;
    if (waves)
        *waves = (a.nstrips * a.nsegs + a.rem_units) *
                 (a.split > 0 ? gol::stream_wpb(a.words, k, s->ilv, s->boundary == GOL_BOUNDED, s->wrap_rows != 0) / 4 : 1);
    return GOL_OK;
}

int strip_step_opts(const gol_strip* s, const uint32_t* src, uint32_t* dst, int k, int64_t out_begin, int64_t out_end,
                    hipStream_t stream, int32_t split_opt, int64_t seg_opt, int32_t seam_opt, int32_t split2_opt) {
    if (int rc = check_strip(s)) return rc;
    if (!src || !dst || src == dst) return fail(GOL_ERR_INVALID, "src and dst must be distinct buffers");
    if (!gol::stream_supported(k, s->ilv)) return fail(GOL_ERR_INVALID, "k not supported for this ilv");
    if (int rc = check_pipe_strip(s, k)) return rc;
    if (out_begin < 0 || out_end > s->rows || out_begin > out_end) return fail(GOL_ERR_INVALID, "bad output rows");
    if (out_begin == out_end) return GOL_OK;
    if (!s->wrap_rows) {
        // every row the pass can read must exist in the buffer, except rows beyond a bounded board's edge
        int64_t lo = out_begin - k, hi = out_end + k;
        if (s->boundary == GOL_BOUNDED) {
            lo = std::max<int64_t>(lo, -s->y0);
            hi = std::min<int64_t>(hi, s->height - s->y0);
        }
        if (lo < -s->ghost || hi > s->rows + s->ghost)
            return fail(GOL_ERR_INVALID, "pass reads rows outside the buffer: ghost must be >= k");
    }
    gol::StreamArgs a = strip_args(s, out_begin, out_end, split_opt, seg_opt, seam_opt, split2_opt);
    GOL_HIP(gol::launch_stream_step(src, dst, a, k, s->boundary == GOL_BOUNDED, s->wrap_rows != 0, stream));
    return GOL_OK;
}

// gol_strip_view_counts with a board's "view_stream" option (the multi board's launches)
int strip_view_counts_opts(const gol_strip* s, const uint32_t* buf, const gol_view* v, uint32_t* dev_counts,
                           hipStream_t stream, bool stream_kernel) {
    if (int rc = check_strip(s)) return rc;
    if (!buf || !dev_counts) return fail(GOL_ERR_INVALID, "null buffer");
    if (int rc = check_view(v, s->width, s->height, s->boundary)) return rc;
    const gol::ViewSource src{buf, s->ilv, s->width, s->height, s->pitch, s->y0, s->rows, s->ghost,
                              s->boundary == GOL_TORUS};
    const gol::ViewArgs a{v->x, v->y, v->scale, v->out_w, v->out_h};
    GOL_HIP(gol::launch_view_counts(src, a, dev_counts, stream_kernel, stream));
    return GOL_OK;
}

}  // namespace gol

extern "C" {

const char* gol_last_error(void) { return g_last_error.c_str(); }

const char* gol_version(void) { return "gol_hip 0.2 (gfx950)"; }

int gol_arch_supported(const char* gcn_arch_name) {
    // gcnArchName is "gfx950" or "gfx950:sramecc+:xnack-": the code object is built for gfx950 only
    if (!gcn_arch_name || std::strncmp(gcn_arch_name, "gfx950", 6) != 0) return 0;
    return gcn_arch_name[6] == '\0' || gcn_arch_name[6] == ':';
}

uint64_t gol_hash_finalize(uint64_t h, int64_t width, int64_t height) {
    auto fmix = [](uint64_t k) {
        k ^= k >> 33;
        k *= 0xff51afd7ed558ccdULL;
        k ^= k >> 33;
        k *= 0xc4ceb9fe1a85ec53ULL;
        k ^= k >> 33;
        return k;
    };
    return fmix(h ^ fmix((uint64_t)width * 0x100000001B3ULL + (uint64_t)height));
}

}  // extern "C"

namespace {

// devices == nullptr: one part on the calling thread's current device
int create_impl(int64_t width, int64_t height, int boundary, const int* devices, int n, int tblock_k, int ilv,
                gol_board** out) {
    try {
        if (!out) return fail(GOL_ERR_INVALID, "null out");
        *out = nullptr;
        if (width < 3 || height < 3)
            return fail(GOL_ERR_INVALID, "width and height must be >= 3 (smaller tori alias neighbours)");
        if (width > ((int64_t)1 << 40) || height > ((int64_t)1 << 40) || width * height > ((int64_t)1 << 42))
            return fail(GOL_ERR_INVALID, "board too large");
        if (boundary != GOL_TORUS && boundary != GOL_BOUNDED) return fail(GOL_ERR_INVALID, "bad boundary");
        if (n < 1 || n > 64) return fail(GOL_ERR_INVALID, "num_gpus must be 1..64");
        if (tblock_k != 0 && !valid_k(tblock_k))
            return fail(GOL_ERR_INVALID, "tblock_k must be 0 (default) or one of 1,2,4,6,8,12,16,24,32");
        if (ilv != 0 && ((ilv != 1 && ilv != 2 && ilv != 4) || width % (32 * ilv)))
            return fail(GOL_ERR_INVALID, "ilv must be 0 (auto) or 1, 2, 4 dividing the width into 32*ilv-cell blocks");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GOL_ERR_NO_DEVICE, "no HIP device");
        if (devices)
            for (int i = 0; i < n; i++)
                if (devices[i] < 0 || devices[i] >= ndev) return fail(GOL_ERR_INVALID, "device index out of range");
        DeviceGuard restore(-1);  // the caller's current device is restored on return
        {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) return fail(GOL_ERR_NO_DEVICE, "no current HIP device");
            for (int i = 0; i < (devices ? n : 1); i++) {
                const int d = devices ? devices[i] : cur;
                hipDeviceProp_t prop;
                if (hipGetDeviceProperties(&prop, d) != hipSuccess)
                    return fail(GOL_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
                if (!gol_arch_supported(prop.gcnArchName))
                    return fail(GOL_ERR_NO_DEVICE, std::string("device ") + std::to_string(d) + " is " +
                                                       prop.gcnArchName + ", this build runs on gfx950 only");
            }
        }
        if (n > 1 && width % 32)
            return fail(GOL_ERR_UNSUPPORTED, "a multi-GPU board needs width % 32 == 0 (bit-packed layout)");
        if (n > 1 && height < n) return fail(GOL_ERR_INVALID, "fewer board rows than GPUs");
        gol_board* b = new gol_board();
        b->W = width;
        b->H = height;
        b->boundary = boundary;
        b->tblock = tblock_k;
        b->packed = (width % 32) == 0;
        b->ilv = b->packed ? (ilv ? ilv : board_ilv(width, height, n, boundary)) : 0;
        // an explicit depth the level-pipelined layout does not run (12, 24 at ilv 4): the streaming layout by width
        if (b->packed && !ilv && tblock_k && !gol::stream_supported(tblock_k, b->ilv)) b->ilv = pick_ilv(width);
        b->tblock = tblock_k ? tblock_k : board_tblock(b->ilv, width * height, boundary);
        if (!b->packed && !tblock_k && ring_by_size(width, height)) {
            // large ragged boards stream as block rows of ring_pitch(W) words: the aligned rules for that many cells
            const int64_t rc = ring_cells(width, height, boundary);
            b->tblock = board_tblock(rc < kSmallBoardCells ? 1 : 2, rc, boundary);
        }
        b->tblock_set = tblock_k != 0;
        b->pitch = b->packed ? width / 32 : 0;
        hipError_t e = devices ? hipSetDevice(devices[0]) : hipSuccess;
        if (e == hipSuccess) e = hipGetDevice(&b->device);
        if (e != hipSuccess) {
            free_board(b);
            return fail(GOL_ERR_HIP, std::string("device: ") + hipGetErrorString(e));
        }
        if (n > 1) {  // row strips over several devices: the multi board owns all device memory
            b->multi = new gol::MultiBoard();
            if (int rc = b->multi->init(width, height, boundary, devices, n, b->tblock, b->ilv)) {
                free_board(b);
                return rc;
            }
            *out = b;
            return GOL_OK;
        }
        e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            free_board(b);
            return fail(GOL_ERR_HIP, std::string("stream: ") + hipGetErrorString(e));
        }
        for (auto& p : b->buf) {
            e = hipMalloc(&p, b->bytes());
            if (e != hipSuccess) {
                free_board(b);
                return fail(GOL_ERR_OOM, std::string("hipMalloc board: ") + hipGetErrorString(e));
            }
        }
        e = hipMalloc(&b->acc, 64);
        if (e == hipSuccess) e = hipMemsetAsync(b->buf[0], 0, b->bytes(), b->stream);
        if (e == hipSuccess) e = hipMemsetAsync(b->buf[1], 0, b->bytes(), b->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
        if (e != hipSuccess) {
            free_board(b);
            return fail(GOL_ERR_HIP, std::string("init: ") + hipGetErrorString(e));
        }
        *out = b;
        return GOL_OK;
    } catch (const std::exception& ex) {
        return fail(GOL_ERR_OOM, ex.what());
    } catch (...) {
        return fail(GOL_ERR_INVALID, "unknown exception");
    }
}

}  // namespace

extern "C" {

int gol_create(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, gol_board** out) {
    return gol_create_ex(width, height, boundary, num_gpus, tblock_k, 0, out);
}

int gol_create_ex(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, int ilv,
                  gol_board** out) {
    if (num_gpus == 1) return create_impl(width, height, boundary, nullptr, 1, tblock_k, ilv, out);
    if (num_gpus < 1 || num_gpus > 64) {
        if (out) *out = nullptr;
        return fail(GOL_ERR_INVALID, "num_gpus must be 1..64");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        if (out) *out = nullptr;
        return fail(GOL_ERR_NO_DEVICE, "no HIP device");
    }
    if (num_gpus > ndev) {
        if (out) *out = nullptr;
        return fail(GOL_ERR_INVALID, "num_gpus exceeds the visible HIP devices (gol_create_multi places strips explicitly)");
    }
    std::vector<int> devs((size_t)num_gpus);
    for (int i = 0; i < num_gpus; i++) devs[(size_t)i] = i;
    return create_impl(width, height, boundary, devs.data(), num_gpus, tblock_k, ilv, out);
}

int gol_create_multi(int64_t width, int64_t height, int boundary, const int* devices, int ndevices, int tblock_k,
                     int ilv, gol_board** out) {
    if (!devices || ndevices < 1) {
        if (out) *out = nullptr;
        return fail(GOL_ERR_INVALID, "devices must list at least one device");
    }
    return create_impl(width, height, boundary, devices, ndevices, tblock_k, ilv, out);
}

int gol_num_parts(gol_board* b, int* n) {
    if (!b || !n) return fail(GOL_ERR_INVALID, "null argument");
    *n = b->multi ? b->multi->parts() : 1;
    return GOL_OK;
}

int gol_part_info(gol_board* b, int part, int* device, int64_t* y0, int64_t* rows, int64_t* ghost) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    const int n = b->multi ? b->multi->parts() : 1;
    if (part < 0 || part >= n) return fail(GOL_ERR_INVALID, "part index out of range");
    if (b->multi) {
        const auto& p = b->multi->part(part);
        if (device) *device = p.device;
        if (y0) *y0 = p.s.y0;
        if (rows) *rows = p.s.rows;
        if (ghost) *ghost = p.s.ghost;
    } else {
        if (device) *device = b->device;
        if (y0) *y0 = 0;
        if (rows) *rows = b->H;
        if (ghost) *ghost = 0;
    }
    return GOL_OK;
}

int gol_transport(gol_board* b, int* transport, char* note, int64_t note_len) {
    if (!b || !transport) return fail(GOL_ERR_INVALID, "null argument");
    std::string n = "single board: no halo exchange";
    *transport = GOL_TRANSPORT_NONE;
    if (b->multi) {
        *transport = b->multi->transport();
        n = b->multi->transport_note();
    }
    if (note && note_len > 0) {
        const size_t len = std::min<size_t>(n.size(), (size_t)note_len - 1);
        std::memcpy(note, n.data(), len);
        note[len] = '\0';
    }
    return GOL_OK;
}

int gol_exchange_plan(int64_t height, int boundary, int nparts, int64_t ghost, int k, gol_xfer* ops, int64_t max_ops,
                      int64_t* n_ops) {
    if (!n_ops || nparts < 2 || height < nparts || k < 1 || ghost < k || (boundary != GOL_TORUS && boundary != GOL_BOUNDED))
        return fail(GOL_ERR_INVALID, "bad exchange plan arguments (nparts >= 2, height >= nparts, ghost >= k >= 1)");
    for (int r = 0; r < nparts; r++)
        if (height * (r + 1) / nparts - height * r / nparts < k) return fail(GOL_ERR_INVALID, "a part is thinner than k");
    try {
        const std::vector<gol_xfer> plan = gol::exchange_plan(height, boundary, nparts, ghost, k);
        *n_ops = (int64_t)plan.size();
        if (ops) {
            if (max_ops < (int64_t)plan.size()) return fail(GOL_ERR_INVALID, "ops array too small");
            std::copy(plan.begin(), plan.end(), ops);
        }
    } catch (const std::exception& ex) {
        return fail(GOL_ERR_OOM, ex.what());
    }
    return GOL_OK;
}

int gol_destroy(gol_board* b) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    DeviceGuard dg(b->device);
    if (b->multi)
        (void)b->multi->synchronize();
    else
        (void)hipStreamSynchronize(b->stream);
    free_board(b);
    return GOL_OK;
}

int gol_set_cells(gol_board* b, const uint8_t* cells, int64_t len) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (!cells || len != b->W * b->H) return fail(GOL_ERR_INVALID, "cells length must be width*height");
    return set_cells_impl(b, cells);
}

int gol_get_cells(gol_board* b, uint8_t* cells, int64_t len) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (!cells || len != b->W * b->H) return fail(GOL_ERR_INVALID, "cells length must be width*height");
    return readback_impl(b, cells, b->W, 1);
}

int gol_get_region(gol_board* b, int64_t x, int64_t y, int64_t w, int64_t h, uint8_t* out) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (!out || x < 0 || y < 0 || w < 0 || h < 0 || x + w > b->W || y + h > b->H)
        return fail(GOL_ERR_INVALID, "region outside the board");
    if (w == 0 || h == 0) return GOL_OK;
    if (b->multi) return b->multi->region(x, y, w, h, out);
    if (int rc = sync_bytes(b)) return rc;
    uint8_t* staging = nullptr;
    hipError_t e = hipMalloc(&staging, (size_t)(w * h));
    if (e != hipSuccess) return fail(GOL_ERR_OOM, "hipMalloc region");
    do {
        e = gol::launch_region(b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->pitch, x, y, w, h, staging, b->stream);
        if (e != hipSuccess) break;
        e = hipMemcpyAsync(out, staging, (size_t)(w * h), hipMemcpyDeviceToHost, b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("get_region: ") + hipGetErrorString(e));
    return check_valid(b);
}

int gol_render_gray8(gol_board* b, uint8_t* pixels, int64_t stride, uint8_t alive_value) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (!pixels || stride < b->W) return fail(GOL_ERR_INVALID, "stride must be >= width");
    return readback_impl(b, pixels, stride, alive_value);
}

uint8_t gol_view_tone(uint32_t count, int64_t scale, int mode, uint8_t alive_value) {
    return gol::view_tone(count, scale, mode, alive_value);
}

// The counts of a view, and with pixels != null their tone map (out_h * stride bytes): one device buffer of counts is
// zeroed, every rectangle of the view adds into it on the board's stream, and only the result crosses to the host.
static int view_impl(gol_board* b, const gol_view* v, uint32_t* counts, int mode, uint8_t alive_value, uint8_t* pixels,
                     int64_t stride) {
    const int64_t n = v->out_w * v->out_h;
    if (b->multi) {
        if (!pixels) return b->multi->view_counts(v, counts, b->opt.view_stream);
        std::vector<uint32_t> host((size_t)n);
        if (int rc = b->multi->view_counts(v, host.data(), b->opt.view_stream)) return rc;
        for (int64_t j = 0; j < v->out_h; j++) {
            uint8_t* row = pixels + j * stride;
            for (int64_t i = 0; i < v->out_w; i++)
                row[i] = gol::view_tone(host[(size_t)(i + j * v->out_w)], v->scale, mode, alive_value);
            std::memset(row + v->out_w, 0, (size_t)(stride - v->out_w));
        }
        return GOL_OK;
    }
    if (int rc = sync_bytes(b)) return rc;  // a ragged board's current generation may live in its scratch rows
    const size_t npix = pixels ? (size_t)(v->out_h * stride) : 0;
    uint32_t* dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), (size_t)n * sizeof(uint32_t) + npix);
    if (e != hipSuccess) return fail(GOL_ERR_OOM, std::string("hipMalloc view: ") + hipGetErrorString(e));
    uint8_t* dev_pixels = reinterpret_cast<uint8_t*>(dev + n);
    do {
        e = hipMemsetAsync(dev, 0, (size_t)n * sizeof(uint32_t) + (stride != v->out_w ? npix : 0), b->stream);
        if (e != hipSuccess) break;
        const gol::ViewSource src{b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->H, b->packed ? b->pitch : b->W, 0,
                                  b->H, 0, b->boundary == GOL_TORUS};
        const gol::ViewArgs a{v->x, v->y, v->scale, v->out_w, v->out_h};
        e = gol::launch_view_counts(src, a, dev, b->opt.view_stream, b->stream);
        if (e != hipSuccess) break;
        if (pixels) {
            e = gol::launch_view_tone(dev, dev_pixels, v->out_w, v->out_h, stride, v->scale, mode, alive_value, b->stream);
            if (e != hipSuccess) break;
            e = hipMemcpyAsync(pixels, dev_pixels, npix, hipMemcpyDeviceToHost, b->stream);
        } else {
            e = hipMemcpyAsync(counts, dev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream);
        }
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("view: ") + hipGetErrorString(e));
    return check_valid(b);
}

int gol_view_counts(gol_board* b, const gol_view* v, uint32_t* counts) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    if (int rc = check_view(v, b->W, b->H, b->boundary)) return rc;
    if (!counts) return fail(GOL_ERR_INVALID, "null counts");
    DeviceGuard dg(b->device);
    return view_impl(b, v, counts, GOL_VIEW_ANY, 0, nullptr, 0);
}

int gol_render_view(gol_board* b, const gol_view* v, int mode, uint8_t alive_value, uint8_t* pixels, int64_t stride) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    if (int rc = check_view(v, b->W, b->H, b->boundary)) return rc;
    if (mode != GOL_VIEW_ANY && mode != GOL_VIEW_DENSITY) return fail(GOL_ERR_INVALID, "view mode must be GOL_VIEW_ANY or GOL_VIEW_DENSITY");
    if (!pixels || stride < v->out_w) return fail(GOL_ERR_INVALID, "stride must be >= out_w");
    DeviceGuard dg(b->device);
    return view_impl(b, v, nullptr, mode, alive_value, pixels, stride);
}

int gol_save_packed(gol_board* b, uint64_t* words, int64_t len) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    const int64_t nc = (b->W + 63) / 64;
    if (!words || len != nc * b->H) return fail(GOL_ERR_INVALID, "words length must be height * ceil(width/64)");
    if (b->multi) return b->multi->save_packed(words);
    if (int rc = sync_bytes(b)) return rc;
    const size_t n = (size_t)len * 8;
    uint64_t* staging = nullptr;
    hipError_t e = hipMalloc(&staging, n);
    if (e != hipSuccess) return fail(GOL_ERR_OOM, "hipMalloc snapshot");
    do {
        e = gol::launch_export_canonical(b->buf[b->cur], b->W, b->H, b->pitch, 0, b->packed ? b->ilv : 0, staging,
                                         b->stream);
        if (e != hipSuccess) break;
        e = hipMemcpyAsync(words, staging, n, hipMemcpyDeviceToHost, b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("save_packed: ") + hipGetErrorString(e));
    return check_valid(b);
}

int gol_load_packed(gol_board* b, const uint64_t* words, int64_t len) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    const int64_t nc = (b->W + 63) / 64;
    if (!words || len != nc * b->H) return fail(GOL_ERR_INVALID, "words length must be height * ceil(width/64)");
    b->generation = 0;
    if (b->multi) return b->multi->load_packed(words);
    const size_t n = (size_t)len * 8;
    uint64_t* staging = nullptr;
    hipError_t e = hipMalloc(&staging, n);
    if (e != hipSuccess) return fail(GOL_ERR_OOM, "hipMalloc snapshot");
    do {
        e = hipMemcpyAsync(staging, words, n, hipMemcpyHostToDevice, b->stream);
        if (e != hipSuccess) break;
        e = gol::launch_import_canonical(staging, b->W, b->H, b->pitch, 0, b->packed ? b->ilv : 0, b->buf[b->cur],
                                         b->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(b->stream);
    } while (0);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("load_packed: ") + hipGetErrorString(e));
    return overwritten(b);
}

int gol_seed_dotnet(gol_board* b, int32_t seed, int mode) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (mode != GOL_INIT_DOTNET_MOD2 && mode != GOL_INIT_DOTNET_NEXT2) return fail(GOL_ERR_INVALID, "bad mode");
    try {
        std::vector<uint8_t> cells((size_t)(b->W * b->H));
        DotNetRandom r(seed);
        // creation order x outer, y inner (GameOfLifeDriver.fs:16-19; Array2D.init in Script.fsx:27)
        for (int64_t x = 0; x < b->W; x++)
            for (int64_t y = 0; y < b->H; y++)
                cells[(size_t)(x + y * b->W)] = (mode == GOL_INIT_DOTNET_MOD2) ? (r.Next() % 2 == 0) : (r.Next(2) == 0);
        b->generation = 0;
        return set_cells_impl(b, cells.data());
    } catch (const std::exception& ex) {
        return fail(GOL_ERR_OOM, ex.what());
    }
}

int gol_seed_splitmix(gol_board* b, uint64_t seed) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (b->multi) {
        b->generation = 0;
        return b->multi->seed_splitmix(seed);
    }
    if (b->packed)
        GOL_HIP(gol::launch_splitmix_packed(b->words(b->cur), b->W / 32, b->H, b->pitch, 0, 0, seed, b->ilv,
                                            b->stream));
    else
        GOL_HIP(gol::launch_splitmix_bytes(b->cells(b->cur), b->W, b->H, seed, b->stream));
    b->generation = 0;
    return overwritten(b);
}

int gol_clear(gol_board* b) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (b->multi) {
        b->generation = 0;
        return b->multi->clear();
    }
    GOL_HIP(hipMemsetAsync(b->buf[b->cur], 0, b->bytes(), b->stream));
    b->generation = 0;
    return overwritten(b);
}

int gol_place_rle(gol_board* b, const char* rle, int64_t x, int64_t y) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    try {
        std::vector<std::pair<int64_t, int64_t>> pts;
        std::string err;
        if (!parse_rle(rle, pts, err)) return fail(GOL_ERR_INVALID, err);
        std::vector<int64_t> xy;
        xy.reserve(pts.size() * 2);
        for (auto& p : pts) {
            xy.push_back((((x + p.first) % b->W) + b->W) % b->W);
            xy.push_back((((y + p.second) % b->H) + b->H) % b->H);
        }
        return place_points(b, xy);
    } catch (const std::exception& ex) {
        return fail(GOL_ERR_OOM, ex.what());
    }
}

int gol_step(gol_board* b, int64_t generations) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (generations < 0) return fail(GOL_ERR_INVALID, "negative generations");
    return step_impl(b, generations);
}

int gol_generation(gol_board* b, int64_t* out) {
    if (!b || !out) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    *out = b->generation;
    return GOL_OK;
}

int gol_synchronize(gol_board* b) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    return sync(b);
}

int gol_population(gol_board* b, int64_t* out) {
    if (int rc = check_board(b)) return rc;
    if (!out) return fail(GOL_ERR_INVALID, "null out");
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    uint64_t v = 0;
    if (int rc = reduce_impl(b, false, &v)) return rc;
    *out = (int64_t)v;
    return GOL_OK;
}

int gol_hash(gol_board* b, uint64_t* out) {
    if (int rc = check_board(b)) return rc;
    if (!out) return fail(GOL_ERR_INVALID, "null out");
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    return reduce_impl(b, true, out);
}

int gol_info(gol_board* b, int64_t* width, int64_t* height, int* boundary, int* tblock_k, int* packed) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    if (width) *width = b->W;
    if (height) *height = b->H;
    if (boundary) *boundary = b->boundary;
    if (tblock_k) *tblock_k = b->tblock;
    if (packed) *packed = b->packed ? 1 : 0;
    return GOL_OK;
}

int gol_layout(gol_board* b, int* ilv, int64_t* pitch) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    if (ilv) *ilv = b->ilv;
    if (pitch) *pitch = b->pitch;
    return GOL_OK;
}

int gol_default_ilv(int64_t width) {
    if (width < 32 || width % 32) return 0;
    return pick_ilv(width);
}

int gol_default_tblock(int ilv) {
    if (ilv != 1 && ilv != 2 && ilv != 4) return 0;
    return default_tblock(ilv);
}

int gol_default_layout(int64_t width, int64_t rows, int boundary, int* ilv, int* tblock_k) {
    if (!ilv || !tblock_k) return fail(GOL_ERR_INVALID, "null argument");
    if (width < 32 || width % 32 || rows < 1 || (boundary != GOL_TORUS && boundary != GOL_BOUNDED))
        return fail(GOL_ERR_INVALID, "width must be a positive multiple of 32, rows >= 1, boundary torus or bounded");
    if (pipe_shape(width, rows, boundary)) {
        *ilv = 4;
        *tblock_k = kPipeK;
    } else {
        *ilv = pick_ilv(width);
        *tblock_k = default_tblock(*ilv);
    }
    return GOL_OK;
}

int gol_supported_k(int k, int ilv) { return gol::stream_supported(k, ilv) ? 1 : 0; }

int gol_pass_timing(gol_board* b, int n, double* interior_us, double* wait_us, double* edge_us) {
    if (int rc = check_board(b)) return rc;
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    const int parts = b->multi ? b->multi->parts() : 1;
    if (n != parts || !interior_us || !wait_us || !edge_us)
        return fail(GOL_ERR_INVALID, "n must equal gol_num_parts and the arrays must be non-null");
    if (b->multi) return b->multi->timed_pass(interior_us, wait_us, edge_us, &b->generation);
    if (!b->packed) return fail(GOL_ERR_UNSUPPORTED, "pass timing needs a bit-packed board");
    // a single board's timed pass is one streaming pass: boards whose gol_step takes another pass are refused, so
    // the figure always describes the pass the board runs
    if (use_wave_resident(b) || use_coop(b) ||
        (b->W * b->H <= resident_max_cells(b) && b->ilv == 1 && gol::resident_packed_fits(b->W, b->H)))
        return fail(GOL_ERR_UNSUPPORTED, "pass timing: this board's gol_step runs the single-wave, cooperative or "
                                         "LDS-resident pass, not the streaming pass the timing measures");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    GOL_HIP(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    const int k = gol::stream_largest_k(b->tblock, b->tblock, b->ilv, b->W / 32, b->boundary == GOL_BOUNDED);
    if (b->ilv == 4 && ensure_err_word(b) != GOL_OK) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipEventRecord(e0, b->stream);
    if (e == hipSuccess) {
        gol::StreamArgs a = b->stream_args(0, b->H, k);
        e = gol::launch_stream_step(b->words(b->cur), b->words(b->cur ^ 1), a, k, b->boundary == GOL_BOUNDED,
                                    b->boundary == GOL_TORUS, b->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(e1, b->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("pass timing: ") + hipGetErrorString(e));
    b->cur ^= 1;
    b->generation += k;
    interior_us[0] = 1e3 * ms;
    wait_us[0] = 0;
    edge_us[0] = 1e3 * ms;
    return GOL_OK;
}

int gol_set_option(gol_board* b, const char* name, int64_t value) {
    if (int rc = check_board(b)) return rc;
    if (!name) return fail(GOL_ERR_INVALID, "null option name");
    std::lock_guard<std::mutex> g(b->mu);
    const std::string n(name);
    BoardOptions& o = b->opt;
    if (n == "coop") o.coop = value != 0;
    else if (n == "coop_k") {
        if (value < 0 || value > 64) return fail(GOL_ERR_INVALID, "coop_k must be 0 (default) .. 64");
        o.coop_k = (int)value;
    } else if (n == "coop_max_cells") o.coop_max_cells = value;
    else if (n == "resident_max_cells") o.resident_max_cells = value;
    else if (n == "wave_resident") o.wave_resident = value != 0;
    else if (n == "split2") {
        if (value < 0 || value >= 65536) return fail(GOL_ERR_INVALID, "split2 must be 0 (engine) .. 65535 (1/65536 units)");
        o.split2 = (int32_t)value;
    } else if (n == "split") {
        if (value >= 65536) return fail(GOL_ERR_INVALID, "split must be < 65536 (1/65536 units; 0 default, < 0 off)");
        o.split = (int32_t)(value < 0 ? -1 : value);
    } else if (n == "seg_rows") o.seg_rows = value < 0 ? 0 : value;
    else if (n == "seam") o.seam = value < 0 ? -1 : 0;
    else if (n == "pipe_split" || n == "pipe_split2") {
        if (value >= 65536) return fail(GOL_ERR_INVALID, n + " must be < 65536 (1/65536 units; 0 default, < 0 equal)");
        (n == "pipe_split" ? o.pipe_split : o.pipe_split2) = (int32_t)(value < 0 ? -1 : value);
    }
    else if (n == "transport") {
        // multi-part boards: 1 = peer copies (the default), 2 = RCCL (distinct devices only)
        if (!b->multi) return fail(GOL_ERR_UNSUPPORTED, "transport: a single board has no halo exchange");
        DeviceGuard dg(b->device);
        return b->multi->set_transport((int)value);
    }
    else if (n == "ragged_stream") o.ragged_stream = value != 0;
    else if (n == "ragged_ring") {
        if (value < 0 || value > 2) return fail(GOL_ERR_INVALID, "ragged_ring must be 0, 1 (by size) or 2");
        o.ragged_ring = (int)value;
    }
    else if (n == "coop_poll_delay") {
        if (value < -1 || value > 4096) return fail(GOL_ERR_INVALID, "coop_poll_delay must be -1 (auto) or 0..4096");
        o.coop_poll_delay = (int)value;
    } else if (n == "lanes") {
        if (value < 0 || value > 2) return fail(GOL_ERR_INVALID, "lanes must be 0, 1 or 2 (by size)");
        o.lanes = (int)value;
    }
    else if (n == "lanes_m") {
        if (value != 0 && value != 3 && value != 5 && value != 9 && value != 17)
            return fail(GOL_ERR_INVALID, "lanes_m must be 0, 3, 5, 9 or 17");
        o.lanes_m = (int)value;
    } else if (n == "view_stream") o.view_stream = value != 0;
    else if (is_debug_option(n))
        return fail(GOL_ERR_INVALID, "'" + n + "' is a test knob (gol_debug_set_option, csrc/gol_debug.h), not a board option");
    else
        return fail(GOL_ERR_INVALID, "unknown option '" + n + "'");
    // a multi-part board runs every strip launch with the streaming options (the other passes never run there)
    if (b->multi) b->multi->set_stream_options(o.split, o.seg_rows, o.seam, o.split2);
    return GOL_OK;
}

// Test and A/B knobs (csrc/gol_debug.h; VERDICT round 4 item 3: kept out of gol.h's option list).
const char* gol_debug_option_names(void) {
    static const std::string names = [] {
        std::string r;
        for (const char* d : kDebugOptions) r += (r.empty() ? "" : ",") + std::string(d);
        return r;
    }();
    return names.c_str();
}

int gol_debug_set_option(gol_board* b, const char* name, int64_t value) {
    if (int rc = check_board(b)) return rc;
    if (!name) return fail(GOL_ERR_INVALID, "null option name");
    std::lock_guard<std::mutex> g(b->mu);
    const std::string n(name);
    BoardOptions& o = b->opt;
    if (n == "coop_r") {
        if (value < 1 || value > 8) return fail(GOL_ERR_INVALID, "coop_r must be 1..8");
        o.coop_r = (int)value;
    } else if (n == "coop_spin_limit") o.coop_spin_limit = value < 0 ? 0 : value;
    else if (n == "coop_launch") o.coop_launch = value != 0;
    else if (n == "resident_threads") {
        if (value != 256 && value != 1024) return fail(GOL_ERR_INVALID, "resident_threads must be 256 or 1024");
        o.resident_threads = (int)value;
    } else if (n == "coop_epoch") {
        // the epoch of the last persistent launch, so the next one runs at value + 1: tests run the 16-bit wrap early.
        // The granules are cleared with it: the buffer may hold granules of any earlier
        // epoch, among them value + 1's own block 0 of parity 0, which would otherwise match the next launch's first
        // poll and hand it stale halo rows.
        if (value < 0 || value > 0xffff) return fail(GOL_ERR_INVALID, "coop_epoch must be 0..65535");
        if (b->coop_xch) {
            DeviceGuard dg(b->device);
            GOL_HIP(hipMemsetAsync(b->coop_xch, 0, (size_t)b->coop_xch_words * sizeof(uint32_t), b->stream));
            b->coop_epoch = (unsigned)value;
        }
    } else if (n == "lanes_launches")
        return fail(GOL_ERR_INVALID, "lanes_launches is read-only");
    else
        return fail(GOL_ERR_INVALID, "unknown debug option '" + n + "'");
    return GOL_OK;
}

int gol_debug_get_option(gol_board* b, const char* name, int64_t* value) {
    if (int rc = check_board(b)) return rc;
    if (!name || !value) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    const std::string n(name);
    const BoardOptions& o = b->opt;
    if (n == "coop_r") *value = o.coop_r;
    else if (n == "coop_spin_limit") *value = o.coop_spin_limit;
    else if (n == "coop_launch") *value = o.coop_launch;
    else if (n == "resident_threads") *value = o.resident_threads;
    else if (n == "coop_epoch") *value = b->coop_epoch;
    else if (n == "lanes_launches") *value = b->lanes_launches;
    else
        return fail(GOL_ERR_INVALID, "unknown debug option '" + n + "'");
    return GOL_OK;
}

int gol_get_option(gol_board* b, const char* name, int64_t* value) {
    if (int rc = check_board(b)) return rc;
    if (!name || !value) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    const std::string n(name);
    const BoardOptions& o = b->opt;
    if (n == "coop") *value = o.coop;
    else if (n == "coop_k") *value = o.coop_k;
    else if (n == "coop_max_cells") *value = o.coop_max_cells;
    else if (n == "resident_max_cells") *value = o.resident_max_cells;
    else if (n == "wave_resident") *value = o.wave_resident;
    else if (n == "split") *value = o.split;
    else if (n == "split2") *value = o.split2;
    else if (n == "seg_rows") *value = o.seg_rows;
    else if (n == "seam") *value = o.seam;
    else if (n == "pipe_split") *value = o.pipe_split;
    else if (n == "pipe_split2") *value = o.pipe_split2;
    else if (n == "ragged_stream") *value = o.ragged_stream;
    else if (n == "ragged_ring") *value = o.ragged_ring;
    else if (n == "coop_poll_delay") *value = o.coop_poll_delay;
    else if (n == "lanes") *value = o.lanes;
    else if (n == "lanes_m") *value = o.lanes_m;
    else if (n == "view_stream") *value = o.view_stream;
    else if (n == "transport") *value = b->multi ? b->multi->transport() : GOL_TRANSPORT_NONE;
    else if (is_debug_option(n))
        return fail(GOL_ERR_INVALID, "'" + n + "' is a test knob (gol_debug_get_option, csrc/gol_debug.h), not a board option");
    else
        return fail(GOL_ERR_INVALID, "unknown option '" + n + "'");
    return GOL_OK;
}

int gol_device_count(int* n) {
    if (!n) return fail(GOL_ERR_INVALID, "null argument");
    *n = 0;
    int c = 0;
    const hipError_t e = hipGetDeviceCount(&c);
    if (e == hipErrorNoDevice) return GOL_OK;
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    *n = c;
    return GOL_OK;
}

int gol_step_timed(gol_board* b, int64_t generations, double* elapsed_us) {
    if (int rc = check_board(b)) return rc;
    if (!elapsed_us) return fail(GOL_ERR_INVALID, "null elapsed_us");
    std::lock_guard<std::mutex> g(b->mu);
    DeviceGuard dg(b->device);
    if (generations < 0) return fail(GOL_ERR_INVALID, "negative generations");
    if (b->multi) return b->multi->step_timed(generations, &b->generation, elapsed_us);
    // before the first event: a ragged board's byte state the call would not use is settled like in gol_step
    hipEvent_t e0 = nullptr, e1 = nullptr;
    GOL_HIP(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    int rc = GOL_OK;
    if (e == hipSuccess) e = hipEventRecord(e0, b->stream);
    if (e == hipSuccess) rc = step_impl(b, generations);
    if (e == hipSuccess && rc == GOL_OK) e = hipEventRecord(e1, b->stream);
    if (e == hipSuccess && rc == GOL_OK) e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess && rc == GOL_OK) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc != GOL_OK) return rc;
    if (e != hipSuccess) return fail(GOL_ERR_HIP, std::string("step timing: ") + hipGetErrorString(e));
    *elapsed_us = 1e3 * ms;
    return check_valid(b);
}

int gol_stream(gol_board* b, void** stream) {
    if (!b || !stream) return fail(GOL_ERR_INVALID, "null argument");
    *stream = (void*)(b->multi ? b->multi->stream0() : b->stream);
    return GOL_OK;
}

// ---------------------------------------------------------------- row strips
int gol_strip_plan(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t* waves, int64_t* seg_rows) {
    return gol::strip_plan_opts(s, k, out_begin, out_end, waves, seg_rows, 0, 0, 0);
}

int gol_strip_plan_ex(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t* plan, int64_t n) {
    if (int rc = check_strip(s)) return rc;
    if (!plan || n < 8) return fail(GOL_ERR_INVALID, "plan needs 8 entries");
    if (!gol::stream_supported(k, s->ilv)) return fail(GOL_ERR_INVALID, "k not supported for this ilv");
    if (s->ilv == 4 && gol::pipe_supported(k))
        return fail(GOL_ERR_UNSUPPORTED, "k = 16 / 32 at ilv 4 is the level-pipelined pass: gol_debug_pipe_plan");
    if (out_begin < 0 || out_end > s->rows || out_begin > out_end) return fail(GOL_ERR_INVALID, "bad output rows");
    gol::StreamArgs a = strip_args(s, out_begin, out_end, 0, 0, 0);
    gol::plan_stream(a, k, s->boundary == GOL_BOUNDED, s->wrap_rows != 0);
    const int64_t v[10] = {a.nstrips, a.nsegs, a.seg, a.seam, a.rem, a.rem_p, a.rem_mid, a.rem_units, a.split, a.split2};
    for (int i = 0; i < (n < 10 ? 8 : 10); i++) plan[i] = v[i];
    return GOL_OK;
}

// The level-pipelined pass's plan for this strip pass with `wgs` resident workgroups (0: the device's), and the
// violations a host walk of it finds (gol_pipe.hip pipe_check_plan): plan[] = nstrips, rem, rq, rp, ngroups, grows,
// pk_lo, pk_hi, npk, nrem, P, split1, split2, grid, violations
int gol_debug_pipe_plan(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t wgs, int64_t* plan,
                        int64_t n) {
    if (int rc = check_strip(s)) return rc;
    if (!plan || n < 15) return fail(GOL_ERR_INVALID, "plan needs 15 entries");
    if (s->ilv != 4 || !gol::pipe_supported(k)) return fail(GOL_ERR_INVALID, "not a level-pipelined pass (ilv 4, k 16 / 32)");
    if (int rc = check_pipe_strip(s, k)) return rc;
    if (out_begin < 0 || out_end > s->rows || out_begin > out_end) return fail(GOL_ERR_INVALID, "bad output rows");
    gol::StreamArgs a = strip_args(s, out_begin, out_end, 0, 0, 0);
    gol::PipeArgs p{};
    p.words = a.words;
    p.pitch = a.pitch;
    p.rows = a.rows;
    p.ghost = a.ghost;
    p.out_begin = out_begin;
    p.out_end = out_end;
    p.spare_waves = a.spare;
    p.wgs_opt = wgs;
    p.bounded = s->boundary == GOL_BOUNDED;
    gol::plan_pipe(p, k, s->wrap_rows != 0, p.spare_waves);
    const int64_t v[15] = {p.nstrips, p.rem, p.rq, p.rp, p.ngroups, p.grows, p.pk_lo, p.pk_hi, p.npk, p.nrem,
                           p.P, p.split1, p.split2, gol::pipe_grid(p), gol::pipe_check_plan(p, k, s->wrap_rows != 0)};
    for (int i = 0; i < 15; i++) plan[i] = v[i];
    return GOL_OK;
}

// Reads and clears the library's own error word of the level-pipelined pass (strip passes; boards use their own)
int gol_debug_pipe_errors(int* out) {
    if (!out) return fail(GOL_ERR_INVALID, "null argument");
    *out = 0;
    int* w = gol::pipe_error_word();
    if (!w) return fail(GOL_ERR_HIP, "no device error word");
    GOL_HIP(hipMemcpy(out, w, sizeof(int), hipMemcpyDeviceToHost));
    GOL_HIP(hipMemset(w, 0, sizeof(int)));
    return GOL_OK;
}

int gol_strip_step(const gol_strip* s, const uint32_t* src, uint32_t* dst, int k, int64_t out_begin,
                   int64_t out_end, void* stream) {
    return gol::strip_step_opts(s, src, dst, k, out_begin, out_end, (hipStream_t)stream, 0, 0, 0);
}

int gol_strip_seed_splitmix(const gol_strip* s, uint32_t* buf, uint64_t seed, void* stream) {
    if (int rc = check_strip(s)) return rc;
    if (!buf) return fail(GOL_ERR_INVALID, "null buffer");
    GOL_HIP(gol::launch_splitmix_packed(buf, s->width / 32, s->rows, s->pitch, s->ghost, s->y0, seed, s->ilv,
                                        (hipStream_t)stream));
    return GOL_OK;
}

int gol_strip_pack(const gol_strip* s, const uint8_t* dev_cells, uint32_t* buf, void* stream) {
    if (int rc = check_strip(s)) return rc;
    if (!dev_cells || !buf) return fail(GOL_ERR_INVALID, "null buffer");
    GOL_HIP(gol::launch_pack(dev_cells, buf, s->width, s->rows, s->pitch, s->ghost, s->ilv, (hipStream_t)stream));
    return GOL_OK;
}

int gol_strip_unpack(const gol_strip* s, const uint32_t* buf, uint8_t* dev_cells, int64_t stride, uint8_t value,
                     void* stream) {
    if (int rc = check_strip(s)) return rc;
    if (!dev_cells || !buf || stride < s->width) return fail(GOL_ERR_INVALID, "bad buffer or stride");
    GOL_HIP(gol::launch_unpack(buf, dev_cells, s->width, s->rows, s->pitch, s->ghost, stride, value, s->ilv,
                               (hipStream_t)stream));
    return GOL_OK;
}

int gol_strip_population(const gol_strip* s, const uint32_t* buf, uint64_t* dev_acc, void* stream) {
    if (int rc = check_strip(s)) return rc;
    if (!buf || !dev_acc) return fail(GOL_ERR_INVALID, "null buffer");
    GOL_HIP(gol::launch_popcount_packed(buf, s->width / 32, s->rows, s->pitch, s->ghost,
                                        (unsigned long long*)dev_acc, (hipStream_t)stream));
    return GOL_OK;
}

int gol_strip_view_counts(const gol_strip* s, const uint32_t* buf, const gol_view* v, uint32_t* dev_counts,
                          void* stream) {
    return gol::strip_view_counts_opts(s, buf, v, dev_counts, (hipStream_t)stream, true);
}

int gol_strip_hash_partial(const gol_strip* s, const uint32_t* buf, uint64_t* dev_acc, void* stream) {
    if (int rc = check_strip(s)) return rc;
    if (!buf || !dev_acc) return fail(GOL_ERR_INVALID, "null buffer");
    GOL_HIP(gol::launch_hash_packed(buf, s->width, s->rows, s->pitch, s->ghost, s->y0, s->ilv,
                                    (unsigned long long*)dev_acc, (hipStream_t)stream));
    return GOL_OK;
}

}  // extern "C"
