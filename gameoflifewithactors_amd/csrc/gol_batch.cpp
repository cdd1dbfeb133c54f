// gol_batch.cpp -- the batch handle of the C ABI (include/gol/gol.h, gol_batch_*): `count` independent boards of one
// single-wave geometry, stepped by one launch with one wavefront per board (gol_batch.hip).
//
// The handle follows the board handle's conventions (gol_capi.cpp): its own mutex and stream, every argument checked
// before any device work, every HIP failure mapped to a GOL_ERR_* code with a thread-local message, no C++ exception
// past an extern "C" function.  The argument arithmetic and the .NET seeding are gol_batch_host.h (host-only).
#include <algorithm>
#include <vector>

#include "gol_batch_host.h"
#include "gol_board.h"
#include "gol_cycle_search.h"
#include "gol_debug.h"
#include "gol_generations.h"
#include "gol_rule.h"

using gol::DeviceBuffer;
using gol::DeviceGuard;
using gol::fail;

struct gol_batch {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t W = 0, H = 0, count = 0;
    int boundary = GOL_TORUS;
    int nw = 0;            // words per row
    int group_waves = 1;   // boards per workgroup (gol_debug_batch_group_waves; DESIGN.md 4.9 has the A/B)
    uint32_t* words = nullptr;  // count * H * nw
    int32_t* cycles = nullptr;  // count * 4 result words of gol_ensemble_cycles, allocated by its first call
    int64_t generation = 0;
    uint32_t rule = gol::kRuleLifePacked;  // birth | survive << 9 (gol_ensemble_set_rule)
    // gol_ensemble_set_rules: one packed rule per board.  rules_host non-empty = per-board mode: the device table
    // `rules` (count words, allocated by the first call, kept until destroy) is the launches' rule source and `rule`
    // is unused; gol_ensemble_set_rule empties rules_host and the batch runs under `rule` again.
    uint32_t* rules = nullptr;
    std::vector<uint32_t> rules_host;
    bool rule_table = false;  // B3/S23 through the rule-table kernels too (gol_debug_batch_rule_table)
    double cycles_us = -1;  // device time of the last census launch (gol_debug_ensemble_cycles_us)
    // Generations (gol_generations.h): fixed at creation.  nstates 2 is the life-like batch: no decay
    // plane, and every launch is the one it was before the family existed.  Above 2, `words` holds 1 + planes arrays of
    // count * H * nw words: the alive plane first, decay plane k at words + (k + 1) * plane_stride().
    int nstates = 2, planes = 0;

    int64_t cells() const { return W * H; }
    int64_t board_words() const { return H * nw; }
    int64_t plane_stride() const { return count * board_words(); }
    uint32_t* board(int64_t i) { return words + i * board_words(); }
    const uint32_t* table() const { return rules_host.empty() ? nullptr : rules; }  // the launchers' `rules`
};

namespace {

constexpr int64_t kStagingBytes = (int64_t)64 << 20;  // cells staged on the device per copy

template <class F>
int with_batch(gol_batch* b, F&& f) {
    if (!b) return fail(GOL_ERR_INVALID, "null batch");
    return gol::guarded([&] {
        std::lock_guard<std::mutex> g(b->mu);
        DeviceGuard dg(b->device);
        return f();
    });
}

void free_batch(gol_batch* b) {
    if (b->words) (void)hipFree(b->words);
    if (b->cycles) (void)hipFree(b->cycles);
    if (b->rules) (void)hipFree(b->rules);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// boards [first, first + n) <-> host bytes, a staging buffer of at most kStagingBytes at a time.  states: the bytes
// are states 0 .. nstates - 1.  Otherwise: in, a byte that is not zero is state 1 and every other cell of the range dead
// (none is left dying); out, 1 for an alive cell and 0 for every other.
int copy_cells(gol_batch* b, int64_t first, int64_t n, const uint8_t* in, uint8_t* out, bool states = false) {
    const int64_t per = std::max<int64_t>(1, kStagingBytes / b->cells());
    DeviceBuffer staging;
    GOL_RC(staging.alloc((size_t)(std::min(per, n) * b->cells())));
    for (int64_t i = 0; i < n; i += per) {
        const int64_t m = std::min(per, n - i);
        const size_t bytes = (size_t)(m * b->cells());
        if (in) {
            GOL_HIP(hipMemcpyAsync(staging.p, in + i * b->cells(), bytes, hipMemcpyHostToDevice, b->stream));
            GOL_HIP(gol::launch_batch_pack(staging.as<uint8_t>(), b->board(first + i), b->plane_stride(), b->W,
                                           m * b->H, b->nstates, states, b->stream));
        } else {
            GOL_HIP(gol::launch_batch_unpack(b->board(first + i), b->plane_stride(), staging.as<uint8_t>(), b->W,
                                             m * b->H, b->W, 1, b->nstates, states, b->stream));
            GOL_HIP(hipMemcpyAsync(out + i * b->cells(), staging.p, bytes, hipMemcpyDeviceToHost, b->stream));
        }
        GOL_HIP(hipStreamSynchronize(b->stream));  // the staging buffer is reused, the host buffer borrowed
    }
    return GOL_OK;
}

// boards [first, first + n) of every decay plane <- 0: what a seeder of the alive plane leaves of the dying cells
int clear_decay(gol_batch* b, int64_t first, int64_t n) {
    for (int k = 1; k <= b->planes; k++)
        GOL_HIP(hipMemsetAsync(b->board(first) + k * b->plane_stride(), 0, (size_t)(n * b->board_words()) * 4,
                               b->stream));
    return GOL_OK;
}

int observe(gol_batch* b, std::vector<unsigned long long>& host) {
    DeviceBuffer acc;
    const size_t bytes = (size_t)b->count * 2 * sizeof(unsigned long long);
    GOL_RC(acc.alloc(bytes, "observables"));
    GOL_HIP(gol::launch_batch_observe(b->words, b->plane_stride(), b->count, b->W, b->H, b->nstates,
                                      acc.as<unsigned long long>(), b->stream));
    host.resize((size_t)b->count * 2);
    GOL_HIP(hipMemcpyAsync(host.data(), acc.p, bytes, hipMemcpyDeviceToHost, b->stream));
    GOL_HIP(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

int create_batch(int64_t width, int64_t height, int boundary, int64_t count, int nstates, gol_batch** out) {
    return gol::guarded([&] {
        if (!out) return fail(GOL_ERR_INVALID, "null out");
        *out = nullptr;
        if (!gol::gen_states_ok(nstates)) return fail(GOL_ERR_INVALID, "nstates must be 2..8");
        if (width < 3 || height < 3)
            return fail(GOL_ERR_INVALID, "width and height must be >= 3 (smaller tori alias neighbours)");
        if (width > ((int64_t)1 << 40) || height > ((int64_t)1 << 40) || width * height > ((int64_t)1 << 42))
            return fail(GOL_ERR_INVALID, "board too large");
        if (boundary != GOL_TORUS && boundary != GOL_BOUNDED) return fail(GOL_ERR_INVALID, "bad boundary");
        if (count < 1 || count > gol::kBatchCountMax) return fail(GOL_ERR_INVALID, "count must be 1..2^22");
        if (!gol::wave_resident_rpl(width, height))
            return fail(GOL_ERR_UNSUPPORTED, "a batch takes the single-wave geometry only: width 3..128 and 1..4 rows "
                                             "per lane on at most 64 lanes (gol_batch_supported)");
        int ndev = 0, cur = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GOL_ERR_NO_DEVICE, "no HIP device");
        if (hipGetDevice(&cur) != hipSuccess) return fail(GOL_ERR_NO_DEVICE, "no current HIP device");
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cur) != hipSuccess)
            return fail(GOL_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
        if (!gol_arch_supported(prop.gcnArchName))
            return fail(GOL_ERR_NO_DEVICE, std::string("device ") + std::to_string(cur) + " is " + prop.gcnArchName +
                                               ", this build runs on gfx950 only");
        gol_batch* b = new gol_batch();
        b->W = width;
        b->H = height;
        b->count = count;
        b->boundary = boundary;
        b->nw = (int)((width + 31) / 32);
        b->device = cur;
        b->nstates = nstates;
        b->planes = gol::gen_planes(nstates);
        hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            free_batch(b);
            return fail(GOL_ERR_HIP, std::string("stream: ") + hipGetErrorString(e));
        }
        const size_t bytes = (size_t)((1 + b->planes) * b->plane_stride()) * sizeof(uint32_t);
        e = hipMalloc(reinterpret_cast<void**>(&b->words), bytes);
        if (e != hipSuccess) {
            b->words = nullptr;
            free_batch(b);
            return fail(GOL_ERR_OOM, std::string("hipMalloc batch: ") + hipGetErrorString(e));
        }
        e = hipMemsetAsync(b->words, 0, bytes, b->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
        if (e != hipSuccess) {
            free_batch(b);
            return fail(GOL_ERR_HIP, std::string("init: ") + hipGetErrorString(e));
        }
        *out = b;
        return GOL_OK;
    });
}

}  // namespace

extern "C" {

int gol_batch_supported(int64_t width, int64_t height) { return gol::wave_resident_rpl(width, height); }

int gol_batch_create(int64_t width, int64_t height, int boundary, int64_t count, gol_batch** out) {
    return create_batch(width, height, boundary, count, 2, out);
}

int gol_generations_create(int64_t width, int64_t height, int boundary, int64_t count, int nstates,
                                 gol_batch** out) {
    return create_batch(width, height, boundary, count, nstates, out);
}

// reads what never changes after creation: no lock
int gol_generations_nstates(gol_batch* b, int* nstates) {
    if (!b || !nstates) return fail(GOL_ERR_INVALID, "null argument");
    *nstates = b->nstates;
    return GOL_OK;
}

int gol_batch_destroy(gol_batch* b) {
    if (!b) return fail(GOL_ERR_INVALID, "null batch");
    DeviceGuard dg(b->device);
    (void)hipStreamSynchronize(b->stream);
    free_batch(b);
    return GOL_OK;
}

// reads what never changes after creation: no lock
int gol_batch_info(gol_batch* b, int64_t* width, int64_t* height, int* boundary, int64_t* count) {
    if (!b) return fail(GOL_ERR_INVALID, "null batch");
    if (width) *width = b->W;
    if (height) *height = b->H;
    if (boundary) *boundary = b->boundary;
    if (count) *count = b->count;
    return GOL_OK;
}

int gol_batch_set_cells(gol_batch* b, int64_t first, int64_t n, const uint8_t* cells, int64_t len) {
    return with_batch(b, [&] {
        if (!cells || !gol::batch_range_ok(first, n, b->count, len, b->cells()))
            return fail(GOL_ERR_INVALID, "boards [first, first + n) must lie in [0, count) and len be n*width*height");
        b->generation = 0;
        return copy_cells(b, first, n, cells, nullptr);
    });
}

int gol_generations_set_states(gol_batch* b, int64_t first, int64_t n, const uint8_t* states, int64_t len) {
    return with_batch(b, [&] {
        if (!states || !gol::batch_range_ok(first, n, b->count, len, b->cells()))
            return fail(GOL_ERR_INVALID, "boards [first, first + n) must lie in [0, count) and len be n*width*height");
        for (int64_t i = 0; i < len; i++)  // before any device work: a refusal leaves the batch as it was
            if (states[i] >= b->nstates)
                return fail(GOL_ERR_INVALID, "a state byte is not below nstates (byte " + std::to_string(i) + ")");
        b->generation = 0;
        return copy_cells(b, first, n, states, nullptr, true);
    });
}

int gol_generations_get_states(gol_batch* b, int64_t first, int64_t n, uint8_t* states, int64_t len) {
    return with_batch(b, [&] {
        if (!states || !gol::batch_range_ok(first, n, b->count, len, b->cells()))
            return fail(GOL_ERR_INVALID, "boards [first, first + n) must lie in [0, count) and len be n*width*height");
        return copy_cells(b, first, n, nullptr, states, true);
    });
}

int gol_batch_get_cells(gol_batch* b, int64_t first, int64_t n, uint8_t* cells, int64_t len) {
    return with_batch(b, [&] {
        if (!cells || !gol::batch_range_ok(first, n, b->count, len, b->cells()))
            return fail(GOL_ERR_INVALID, "boards [first, first + n) must lie in [0, count) and len be n*width*height");
        return copy_cells(b, first, n, nullptr, cells);
    });
}

int gol_batch_seed_dotnet(gol_batch* b, const int32_t* seeds, int64_t n, int mode) {
    return with_batch(b, [&] {
        if (!seeds || n != b->count) return fail(GOL_ERR_INVALID, "seeds must hold count entries");
        if (mode != GOL_INIT_DOTNET_MOD2 && mode != GOL_INIT_DOTNET_NEXT2) return fail(GOL_ERR_INVALID, "bad mode");
        // packed on the host, a bounded number of boards per copy
        const int64_t bw = b->board_words();
        const int64_t per = std::max<int64_t>(1, kStagingBytes / (bw * 4));
        std::vector<uint32_t> host((size_t)(std::min(per, n) * bw));
        b->generation = 0;
        for (int64_t i = 0; i < n; i += per) {
            const int64_t m = std::min(per, n - i);
            for (int64_t k = 0; k < m; k++)
                gol::batch_seed_dotnet_words(seeds[i + k], mode, b->W, b->H, host.data() + k * bw);
            GOL_HIP(hipMemcpyAsync(b->board(i), host.data(), (size_t)(m * bw) * 4, hipMemcpyHostToDevice, b->stream));
            GOL_HIP(hipStreamSynchronize(b->stream));
        }
        return clear_decay(b, 0, b->count);
    });
}

int gol_batch_seed_splitmix(gol_batch* b, uint64_t seed) {
    return with_batch(b, [&] {
        GOL_HIP(gol::launch_batch_splitmix(b->words, b->count, b->W, b->H, seed, b->stream));
        b->generation = 0;
        return clear_decay(b, 0, b->count);
    });
}

int gol_batch_clear(gol_batch* b) {
    return with_batch(b, [&] {
        GOL_HIP(hipMemsetAsync(b->words, 0, (size_t)((1 + b->planes) * b->plane_stride()) * 4, b->stream));
        b->generation = 0;
        return GOL_OK;
    });
}

int gol_batch_step(gol_batch* b, int64_t generations) {
    return with_batch(b, [&] {
        if (generations < 0) return fail(GOL_ERR_INVALID, "generations must be >= 0");
        if (generations == 0) return GOL_OK;
        GOL_HIP(gol::launch_batch_step(b->words, b->count, b->W, b->H, b->boundary == GOL_BOUNDED, 1, generations,
                                      nullptr, b->group_waves, b->rule, b->rule_table, b->table(), b->nstates,
                                      b->stream));
        b->generation += generations;
        return GOL_OK;
    });
}

int gol_batch_step_timed(gol_batch* b, int64_t generations, double* elapsed_us) {
    return with_batch(b, [&] {
        if (!elapsed_us) return fail(GOL_ERR_INVALID, "null elapsed_us");
        if (generations < 0) return fail(GOL_ERR_INVALID, "generations must be >= 0");
        gol::EventPair ev;
        GOL_RC(ev.create());
        GOL_HIP(hipEventRecord(ev.e0, b->stream));
        if (generations > 0)
            GOL_HIP(gol::launch_batch_step(b->words, b->count, b->W, b->H, b->boundary == GOL_BOUNDED, 1, generations,
                                          nullptr, b->group_waves, b->rule, b->rule_table, b->table(), b->nstates,
                                          b->stream));
        GOL_HIP(hipEventRecord(ev.e1, b->stream));
        b->generation += generations;
        return ev.elapsed_us(elapsed_us);
    });
}

int gol_batch_step_trace(gol_batch* b, int64_t generations, int64_t every, uint32_t* trace, int64_t len) {
    return with_batch(b, [&] {
        int64_t samples = 0;
        const char* why = "";
        if (!gol::batch_trace_ok(generations, every, b->count, len, &samples, &why)) return fail(GOL_ERR_INVALID, why);
        if (samples == 0) return GOL_OK;
        if (!trace) return fail(GOL_ERR_INVALID, "null trace");
        DeviceBuffer dev;
        const size_t bytes = (size_t)len * sizeof(uint32_t);
        GOL_RC(dev.alloc(bytes, "trace"));
        GOL_HIP(gol::launch_batch_step(b->words, b->count, b->W, b->H, b->boundary == GOL_BOUNDED, samples, every,
                                      dev.as<uint32_t>(), b->group_waves, b->rule, b->rule_table, b->table(), b->nstates,
                                      b->stream));
        b->generation += generations;
        GOL_HIP(hipMemcpyAsync(trace, dev.p, bytes, hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return GOL_OK;
    });
}

int gol_batch_generation(gol_batch* b, int64_t* out) {
    if (!b || !out) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    *out = b->generation;
    return GOL_OK;
}

int gol_batch_populations(gol_batch* b, int64_t* out, int64_t n) {
    return with_batch(b, [&] {
        if (!out || n != b->count) return fail(GOL_ERR_INVALID, "out must hold count entries");
        std::vector<unsigned long long> host;
        GOL_RC(observe(b, host));
        for (int64_t i = 0; i < n; i++) out[i] = (int64_t)host[(size_t)(2 * i)];
        return GOL_OK;
    });
}

int gol_batch_hashes(gol_batch* b, uint64_t* out, int64_t n) {
    return with_batch(b, [&] {
        if (!out || n != b->count) return fail(GOL_ERR_INVALID, "out must hold count entries");
        std::vector<unsigned long long> host;
        GOL_RC(observe(b, host));
        for (int64_t i = 0; i < n; i++) out[i] = gol_hash_finalize(host[(size_t)(2 * i + 1)], b->W, (b->nstates - 1) * b->H);
        return GOL_OK;
    });
}

int gol_batch_render_gray8(gol_batch* b, int64_t board, uint8_t* pixels, int64_t stride, uint8_t alive_value) {
    return with_batch(b, [&] {
        if (board < 0 || board >= b->count) return fail(GOL_ERR_INVALID, "board index outside [0, count)");
        if (!pixels || stride < b->W) return fail(GOL_ERR_INVALID, "stride must be >= width");
        const size_t n = (size_t)(stride * b->H);
        DeviceBuffer staging;
        GOL_RC(staging.alloc(n));
        if (stride != b->W) GOL_HIP(hipMemsetAsync(staging.p, 0, n, b->stream));
        GOL_HIP(gol::launch_batch_unpack(b->board(board), b->plane_stride(), staging.as<uint8_t>(), b->W, b->H, stride,
                                         alive_value, b->nstates, false, b->stream));
        GOL_HIP(hipMemcpyAsync(pixels, staging.p, n, hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return GOL_OK;
    });
}

int gol_ensemble_cycles(gol_batch* b, int64_t max_generations, int64_t* transient, int64_t* period,
                        int64_t* population, int64_t* steps, int64_t n) {
    return with_batch(b, [&] {
        if (!transient || !period || !population || n != b->count)
            return fail(GOL_ERR_INVALID, "transient, period and population must hold count entries");
        if (max_generations < 1 || max_generations > gol::kCycleGenerationsMax)
            return fail(GOL_ERR_INVALID, "max_generations must be 1..2^20");
        static_assert(gol::kBatchCountMax * 4 * (int64_t)sizeof(int32_t) <= kStagingBytes, "one copy of the results");
        const size_t bytes = (size_t)b->count * 4 * sizeof(int32_t);
        if (!b->cycles) {
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->cycles), bytes);
            if (e != hipSuccess) {
                b->cycles = nullptr;
                return fail(GOL_ERR_OOM, std::string("hipMalloc cycle results: ") + hipGetErrorString(e));
            }
        }
        std::vector<int32_t> host((size_t)b->count * 4);
        gol::EventPair ev;
        GOL_RC(ev.create());
        GOL_HIP(hipEventRecord(ev.e0, b->stream));
        GOL_HIP(gol::launch_batch_cycles(b->words, b->count, b->W, b->H, b->boundary == GOL_BOUNDED, max_generations,
                                         b->cycles, b->rule, b->rule_table, b->table(), b->nstates, b->stream));
        GOL_HIP(hipEventRecord(ev.e1, b->stream));
        GOL_HIP(hipMemcpyAsync(host.data(), b->cycles, bytes, hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        GOL_RC(ev.elapsed_us(&b->cycles_us));
        for (int64_t i = 0; i < n; i++) {  // the caller's arrays are written only once every device call succeeded
            const int32_t* r = host.data() + 4 * i;
            transient[i] = r[0];
            period[i] = r[1];
            population[i] = r[2];
            if (steps) steps[i] = r[3];
        }
        return GOL_OK;
    });
}

int gol_rule_parse(const char* text, int* birth, int* survive) {
    const char* why = "";
    return gol::rule_parse(text, birth, survive, &why) ? GOL_OK : fail(GOL_ERR_INVALID, std::string("rule: ") + why);
}

int gol_rule_format(int birth, int survive, char* out, int64_t len) {
    const char* why = "";
    return gol::rule_format(birth, survive, out, len, &why) ? GOL_OK : fail(GOL_ERR_INVALID, std::string("rule: ") + why);
}

int gol_generations_parse(const char* text, int* birth, int* survive, int* nstates) {
    const char* why = "";
    return gol::generations_parse(text, birth, survive, nstates, &why) ? GOL_OK
                                                                       : fail(GOL_ERR_INVALID, std::string("rule: ") + why);
}

int gol_generations_format(int birth, int survive, int nstates, char* out, int64_t len) {
    const char* why = "";
    return gol::generations_format(birth, survive, nstates, out, len, &why)
               ? GOL_OK
               : fail(GOL_ERR_INVALID, std::string("rule: ") + why);
}

int gol_ensemble_set_rule(gol_batch* b, int birth, int survive) {
    return with_batch(b, [&] {
        if (!gol::rule_masks_ok(birth, survive))
            return fail(GOL_ERR_INVALID, "birth and survive masks must lie in 0..0x1FF");
        b->rule = gol::rule_pack(birth, survive);
        b->rules_host.clear();  // one rule for every board again: the kernels and arguments of a batch without a table
        return GOL_OK;
    });
}

int gol_ensemble_rule(gol_batch* b, int* birth, int* survive) {
    if (!b) return fail(GOL_ERR_INVALID, "null batch");
    std::lock_guard<std::mutex> g(b->mu);
    uint32_t rule = b->rule;
    if (!b->rules_host.empty() && !gol::batch_rules_common(b->rules_host.data(), b->count, &rule))
        return fail(GOL_ERR_UNSUPPORTED, "the boards of this batch run under different rules: gol_ensemble_rules "
                                         "returns the table");
    if (birth) *birth = (int)(rule & gol::kRuleMaskMax);
    if (survive) *survive = (int)(rule >> 9);
    return GOL_OK;
}

int gol_ensemble_set_rules(gol_batch* b, const int* birth, const int* survive, int64_t n) {
    return with_batch(b, [&] {
        // the whole table is judged and packed before the device hears of it: a refusal leaves the rules as they were
        const char* why = "";
        int64_t bad = -1;
        std::vector<uint32_t> packed((size_t)b->count);
        if (!gol::batch_rules_pack(birth, survive, n, b->count, packed.data(), &why, &bad))
            return fail(GOL_ERR_INVALID, bad < 0 ? std::string(why) : why + (" (board " + std::to_string(bad) + ")"));
        const size_t bytes = (size_t)b->count * sizeof(uint32_t);
        if (!b->rules) {
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->rules), bytes);
            if (e != hipSuccess) {
                b->rules = nullptr;
                return fail(GOL_ERR_OOM, std::string("hipMalloc rule table: ") + hipGetErrorString(e));
            }
        }
        // on the batch's stream: after every step launched so far, before every later one
        GOL_HIP(hipMemcpyAsync(b->rules, packed.data(), bytes, hipMemcpyHostToDevice, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));  // `packed` is borrowed by the copy
        b->rules_host.swap(packed);
        return GOL_OK;
    });
}

int gol_ensemble_rules(gol_batch* b, int* birth, int* survive, int64_t n) {
    if (!b) return fail(GOL_ERR_INVALID, "null batch");
    std::lock_guard<std::mutex> g(b->mu);
    if (n != b->count) return fail(GOL_ERR_INVALID, "birth and survive hold count entries");
    for (int64_t i = 0; i < n; i++) {
        const uint32_t rule = b->rules_host.empty() ? b->rule : b->rules_host[(size_t)i];
        if (birth) birth[i] = (int)(rule & gol::kRuleMaskMax);
        if (survive) survive[i] = (int)(rule >> 9);
    }
    return GOL_OK;
}

int gol_batch_synchronize(gol_batch* b) {
    return with_batch(b, [&] {
        GOL_HIP(hipStreamSynchronize(b->stream));
        return GOL_OK;
    });
}

int gol_debug_batch_group_waves(gol_batch* b, int waves) {
    return with_batch(b, [&] {
        if (waves != 1 && waves != 4) return fail(GOL_ERR_INVALID, "waves per workgroup must be 1 or 4");
        b->group_waves = waves;
        return GOL_OK;
    });
}

int gol_debug_batch_rule_table(gol_batch* b, int force) {
    return with_batch(b, [&] {
        if (force != 0 && force != 1) return fail(GOL_ERR_INVALID, "force must be 0 or 1");
        b->rule_table = force == 1;
        return GOL_OK;
    });
}

int gol_debug_ensemble_cycles_us(gol_batch* b, double* elapsed_us) {
    return with_batch(b, [&] {
        if (!elapsed_us) return fail(GOL_ERR_INVALID, "null elapsed_us");
        if (b->cycles_us < 0) return fail(GOL_ERR_INVALID, "no gol_ensemble_cycles call on this batch yet");
        *elapsed_us = b->cycles_us;
        return GOL_OK;
    });
}

}  // extern "C"
