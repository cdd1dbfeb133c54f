// gol_capi.cpp -- the C ABI (include/gol/gol.h): board handles, seeding, stepping, readback.
//
// This file is the native runtime around the kernels: it owns a board's device memory, moves cells in and out of it,
// and maps every HIP failure to a GOL_ERR_* code with a thread-local message.  No C++ exception escapes an extern "C"
// function: every entry point that works on a board goes through gol::with_board (gol_board.h).  Stepping is
// gol_passes.cpp (the pass is chosen in gol_policy.cpp), the row strip primitives gol_strip.cpp, the options
// gol_options.cpp.
#include <algorithm>
#include <cstring>
#include <vector>

#include "gol_board.h"
#include "gol_hash.h"
#include "gol_rule.h"
#include "gol_seed_rle.h"
#include "gol_view.h"

using gol::DeviceBuffer;
using gol::check_valid;
using gol::DeviceGuard;
using gol::fail;
using gol::kCoopErrWord;
using gol::sync_bytes;
using gol::with_board;

namespace {

thread_local std::string g_last_error;

// temporal-block depths accepted as a cap (gol_create's tblock_k); each layout supports a subset
bool valid_k(int k) {
    return k == 1 || k == 2 || k == 4 || k == 6 || k == 8 || k == 12 || k == 16 || k == 24 || k == 32;
}

}  // namespace

namespace gol {

int api_fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
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

// A ragged byte board whose state the multi-generation passes left in the scratch rows (rag_state): unpack it into
// the bytes, on the board's stream, before anything reads or modifies them.
int sync_bytes(gol_board* b) {
    if (!b->rag_state) return GOL_OK;
    if (b->rag_state == 3)
        GOL_HIP(gol::launch_unpack_ring(b->rag[b->rag_cur], b->cells(b->cur), b->W, b->H, b->rag_ilv,
                                        b->boundary == GOL_TORUS, b->stream));
    else
        GOL_HIP(gol::launch_unpack_ragged(b->rag[b->rag_cur], b->cells(b->cur), b->W, b->H, b->rag_pitch, b->stream));
    if (b->rag_state == 4)  // a Generations board: the decay planes behind the alive rows become the d bytes
        GOL_HIP(gol::launch_unpack_ragged_decay(b->rag[b->rag_cur] + b->rag_pitch * b->H, b->dec_cells(b->cur), b->W, b->H,
                                                b->rag_pitch, gol::gen_planes(b->nstates), b->stream));
    b->rag_state = 0;
    return GOL_OK;
}

}  // namespace gol

namespace {

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
//
// A Generations board (nstates > 2): everything that overwrites cells writes the alive plane alone, and this is the one
// place where every decay word becomes zero behind it (set_cells, load_packed, the seeds, clear).  gol_set_states
// writes the decay itself (clear_decay = false).
int overwritten(gol_board* b, bool clear_decay = true) {
    if (!b->multi) {
        if (clear_decay && b->dec[b->cur]) GOL_HIP(hipMemsetAsync(b->dec[b->cur], 0, b->dec_bytes(), b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        if (b->coop) {
            GOL_HIP(hipMemsetAsync(b->coop + kCoopErrWord, 0, sizeof(unsigned), b->stream));
            GOL_HIP(hipStreamSynchronize(b->stream));
        }
    }
    b->invalid = b->invalid_pipe = false;
    b->rag_state = 0;
    return b->multi ? b->multi->synchronize() : GOL_OK;
}

int set_cells_impl(gol_board* b, const uint8_t* host) {
    if (b->multi) return b->multi->set_cells(host);
    const size_t n = (size_t)(b->W * b->H);
    if (!b->packed) {
        GOL_HIP(hipMemcpyAsync(b->cells(b->cur), host, n, hipMemcpyHostToDevice, b->stream));
        return overwritten(b);
    }
    DeviceBuffer staging;
    GOL_RC(staging.alloc(n));
    GOL_HIP(hipMemcpyAsync(staging.p, host, n, hipMemcpyHostToDevice, b->stream));
    GOL_HIP(gol::launch_pack(staging.as<uint8_t>(), b->words(b->cur), b->W, b->H, b->pitch, 0, b->ilv, b->stream));
    GOL_HIP(hipStreamSynchronize(b->stream));
    return overwritten(b);
}

int readback_impl(gol_board* b, uint8_t* host, int64_t stride, uint8_t value) {
    if (b->multi) return b->multi->readback(host, stride, value);
    GOL_RC(sync_bytes(b));
    const size_t n = (size_t)(stride * b->H);
    DeviceBuffer staging;
    GOL_RC(staging.alloc(n));
    if (stride != b->W) GOL_HIP(hipMemsetAsync(staging.p, 0, n, b->stream));
    if (b->packed)
        GOL_HIP(gol::launch_unpack(b->words(b->cur), staging.as<uint8_t>(), b->W, b->H, b->pitch, 0, stride, value,
                                   b->ilv, b->stream));
    else
        GOL_HIP(gol::launch_bytes_render(b->cells(b->cur), staging.as<uint8_t>(), b->W, b->H, stride, value, b->stream));
    GOL_HIP(hipMemcpyAsync(host, staging.p, n, hipMemcpyDeviceToHost, b->stream));
    GOL_HIP(hipStreamSynchronize(b->stream));
    return check_valid(b);
}

int reduce_impl(gol_board* b, bool hash, uint64_t* out) {
    if (b->multi) return b->multi->reduce(hash, out);
    GOL_RC(sync_bytes(b));
    GOL_HIP(hipMemsetAsync(b->acc, 0, sizeof(unsigned long long), b->stream));
    const bool stacked = hash && b->nstates > 2;  // a Generations board: the hash of the stacked board (gol.h)
    if (stacked) {
        GOL_HIP(gol::launch_gen_hash(b->buf[b->cur], b->dec[b->cur], b->packed ? b->ilv : 0, b->W, b->H, b->pitch,
                                     b->nstates, b->acc, b->stream));
    } else if (b->packed) {
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
    GOL_RC(check_valid(b));
    *out = hash ? gol_hash_finalize(v, b->W, stacked ? (b->nstates - 1) * b->H : b->H) : (uint64_t)v;
    return GOL_OK;
}

int place_points(gol_board* b, const std::vector<int64_t>& xy) {
    const int64_t n = (int64_t)xy.size() / 2;
    if (n == 0) return GOL_OK;
    if (b->multi) return b->multi->place_points(xy);
    GOL_RC(sync_bytes(b));
    DeviceBuffer d;
    GOL_RC(d.alloc(xy.size() * sizeof(int64_t), "points"));
    GOL_HIP(hipMemcpyAsync(d.p, xy.data(), xy.size() * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
    GOL_HIP(gol::launch_set_points(b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->pitch, d.as<int64_t>(), n, b->stream));
    if (b->nstates > 2)  // a placed cell is in state 1: the alive plane and the decay stay exclusive
        GOL_HIP(gol::launch_clear_points_decay(b->dec[b->cur], b->packed ? b->ilv : 0, b->W, b->H, b->pitch, b->nstates,
                                               d.as<int64_t>(), n, b->stream));
    GOL_HIP(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

void free_board(gol_board* b) {
    delete b->multi;
    for (auto& p : b->buf)
        if (p) (void)hipFree(p);
    for (auto& p : b->dec)
        if (p) (void)hipFree(p);
    if (b->acc) (void)hipFree(b->acc);
    if (b->coop) (void)hipFree(b->coop);
    if (b->coop_xch) (void)hipFree(b->coop_xch);
    for (uint32_t* r : b->rag)
        if (r) (void)hipFree(r);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// devices == nullptr: one part on the calling thread's current device
int create_impl(int64_t width, int64_t height, int boundary, const int* devices, int n, int tblock_k, int ilv,
                gol_board** out) {
    return gol::guarded([&] {
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
        gol::board_layout(b, n, tblock_k, ilv);
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
    });
}

// The counts of a view, and with pixels != null their tone map (out_h * stride bytes): one device buffer of counts is
// zeroed, every rectangle of the view adds into it on the board's stream, and only the result crosses to the host.
int view_impl(gol_board* b, const gol_view* v, uint32_t* counts, int mode, uint8_t alive_value, uint8_t* pixels,
              int64_t stride) {
    const int64_t n = v->out_w * v->out_h;
    if (b->multi) {
        if (!pixels) return b->multi->view_counts(v, counts, b->opt.view_stream);
        std::vector<uint32_t> host((size_t)n);
        GOL_RC(b->multi->view_counts(v, host.data(), b->opt.view_stream));
        for (int64_t j = 0; j < v->out_h; j++) {
            uint8_t* row = pixels + j * stride;
            for (int64_t i = 0; i < v->out_w; i++)
                row[i] = gol::view_tone(host[(size_t)(i + j * v->out_w)], v->scale, mode, alive_value);
            std::memset(row + v->out_w, 0, (size_t)(stride - v->out_w));
        }
        return GOL_OK;
    }
    GOL_RC(sync_bytes(b));  // a ragged board's current generation may live in its scratch rows
    const size_t ncount = (size_t)n * sizeof(uint32_t), npix = pixels ? (size_t)(v->out_h * stride) : 0;
    DeviceBuffer buf;
    GOL_RC(buf.alloc(ncount + npix, "view"));
    uint32_t* dev = buf.as<uint32_t>();
    uint8_t* dev_pixels = reinterpret_cast<uint8_t*>(dev + n);
    GOL_HIP(hipMemsetAsync(dev, 0, ncount + (stride != v->out_w ? npix : 0), b->stream));
    const gol::ViewSource src{b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->H, b->packed ? b->pitch : b->W, 0,
                              b->H, 0, b->boundary == GOL_TORUS};
    const gol::ViewArgs a{v->x, v->y, v->scale, v->out_w, v->out_h};
    GOL_HIP(gol::launch_view_counts(src, a, dev, b->opt.view_stream, b->stream));
    if (pixels) {
        GOL_HIP(gol::launch_view_tone(dev, dev_pixels, v->out_w, v->out_h, stride, v->scale, mode, alive_value, b->stream));
        GOL_HIP(hipMemcpyAsync(pixels, dev_pixels, npix, hipMemcpyDeviceToHost, b->stream));
    } else {
        GOL_HIP(hipMemcpyAsync(counts, dev, ncount, hipMemcpyDeviceToHost, b->stream));
    }
    GOL_HIP(hipStreamSynchronize(b->stream));
    return check_valid(b);
}

}  // namespace

extern "C" {

const char* gol_last_error(void) { return g_last_error.c_str(); }

const char* gol_version(void) { return "gol_hip 0.2 (gfx950)"; }

int gol_arch_supported(const char* gcn_arch_name) {
    // gcnArchName is "gfx950" or "gfx950:sramecc+:xnack-": the code object is built for gfx950 only
    if (!gcn_arch_name || std::strncmp(gcn_arch_name, "gfx950", 6) != 0) return 0;
    return gcn_arch_name[6] == '\0' || gcn_arch_name[6] == ':';
}

uint64_t gol_hash_finalize(uint64_t h, int64_t width, int64_t height) {
    return gol::fmix64(h ^ gol::fmix64((uint64_t)width * 0x100000001B3ULL + (uint64_t)height));
}

int gol_create(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, gol_board** out) {
    return gol_create_ex(width, height, boundary, num_gpus, tblock_k, 0, out);
}

int gol_create_ex(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, int ilv,
                  gol_board** out) {
    if (num_gpus == 1) return create_impl(width, height, boundary, nullptr, 1, tblock_k, ilv, out);
    if (out) *out = nullptr;
    if (num_gpus < 1 || num_gpus > 64) return fail(GOL_ERR_INVALID, "num_gpus must be 1..64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(GOL_ERR_NO_DEVICE, "no HIP device");
    if (num_gpus > ndev)
        return fail(GOL_ERR_INVALID, "num_gpus exceeds the visible HIP devices (gol_create_multi places strips explicitly)");
    int devs[64];
    for (int i = 0; i < num_gpus; i++) devs[i] = i;
    return create_impl(width, height, boundary, devs, num_gpus, tblock_k, ilv, out);
}

int gol_create_multi(int64_t width, int64_t height, int boundary, const int* devices, int ndevices, int tblock_k,
                     int ilv, gol_board** out) {
    if (!devices || ndevices < 1) {
        if (out) *out = nullptr;
        return fail(GOL_ERR_INVALID, "devices must list at least one device");
    }
    return create_impl(width, height, boundary, devices, ndevices, tblock_k, ilv, out);
}

// gol_num_parts, gol_part_info, gol_info, gol_layout and gol_stream read what never changes after creation and take no
// lock: callers may poll them while a step runs.
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

int gol_stream(gol_board* b, void** stream) {
    if (!b || !stream) return fail(GOL_ERR_INVALID, "null argument");
    *stream = (void*)(b->multi ? b->multi->stream0() : b->stream);
    return GOL_OK;
}

int gol_transport(gol_board* b, int* transport, char* note, int64_t note_len) {
    if (!b || !transport) return fail(GOL_ERR_INVALID, "null argument");
    const char* n = "single board: no halo exchange";
    *transport = GOL_TRANSPORT_NONE;
    if (b->multi) {
        *transport = b->multi->transport();
        n = b->multi->transport_note().c_str();
    }
    if (note && note_len > 0) {
        const size_t len = std::min<size_t>(std::strlen(n), (size_t)note_len - 1);
        std::memcpy(note, n, len);
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
    return gol::guarded([&] {
        const std::vector<gol_xfer> plan = gol::exchange_plan(height, boundary, nparts, ghost, k);
        *n_ops = (int64_t)plan.size();
        if (ops) {
            if (max_ops < (int64_t)plan.size()) return fail(GOL_ERR_INVALID, "ops array too small");
            std::copy(plan.begin(), plan.end(), ops);
        }
        return GOL_OK;
    });
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
    return with_board(b, [&] {
        if (!cells || len != b->W * b->H) return fail(GOL_ERR_INVALID, "cells length must be width*height");
        b->generation = 0;  // a new board, as after every other setter (gol.h)
        return set_cells_impl(b, cells);
    });
}

int gol_get_cells(gol_board* b, uint8_t* cells, int64_t len) {
    return with_board(b, [&] {
        if (!cells || len != b->W * b->H) return fail(GOL_ERR_INVALID, "cells length must be width*height");
        return readback_impl(b, cells, b->W, 1);
    });
}

int gol_get_region(gol_board* b, int64_t x, int64_t y, int64_t w, int64_t h, uint8_t* out) {
    return with_board(b, [&] {
        if (!out || x < 0 || y < 0 || w < 0 || h < 0 || x + w > b->W || y + h > b->H)
            return fail(GOL_ERR_INVALID, "region outside the board");
        if (w == 0 || h == 0) return GOL_OK;
        if (b->multi) return b->multi->region(x, y, w, h, out);
        GOL_RC(sync_bytes(b));
        DeviceBuffer staging;
        GOL_RC(staging.alloc((size_t)(w * h), "region"));
        GOL_HIP(gol::launch_region(b->buf[b->cur], b->packed ? b->ilv : 0, b->W, b->pitch, x, y, w, h,
                                   staging.as<uint8_t>(), b->stream));
        GOL_HIP(hipMemcpyAsync(out, staging.p, (size_t)(w * h), hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return check_valid(b);
    });
}

int gol_render_gray8(gol_board* b, uint8_t* pixels, int64_t stride, uint8_t alive_value) {
    return with_board(b, [&] {
        if (!pixels || stride < b->W) return fail(GOL_ERR_INVALID, "stride must be >= width");
        return readback_impl(b, pixels, stride, alive_value);
    });
}

uint8_t gol_view_tone(uint32_t count, int64_t scale, int mode, uint8_t alive_value) {
    return gol::view_tone(count, scale, mode, alive_value);
}

int gol_view_counts(gol_board* b, const gol_view* v, uint32_t* counts) {
    return with_board(b, [&] {
        GOL_RC(gol::check_view(v, b->W, b->H, b->boundary));
        if (!counts) return fail(GOL_ERR_INVALID, "null counts");
        return view_impl(b, v, counts, GOL_VIEW_ANY, 0, nullptr, 0);
    });
}

int gol_render_view(gol_board* b, const gol_view* v, int mode, uint8_t alive_value, uint8_t* pixels, int64_t stride) {
    return with_board(b, [&] {
        GOL_RC(gol::check_view(v, b->W, b->H, b->boundary));
        if (mode != GOL_VIEW_ANY && mode != GOL_VIEW_DENSITY) return fail(GOL_ERR_INVALID, "view mode must be GOL_VIEW_ANY or GOL_VIEW_DENSITY");
        if (!pixels || stride < v->out_w) return fail(GOL_ERR_INVALID, "stride must be >= out_w");
        return view_impl(b, v, nullptr, mode, alive_value, pixels, stride);
    });
}

int gol_save_packed(gol_board* b, uint64_t* words, int64_t len) {
    return with_board(b, [&] {
        const int64_t nc = (b->W + 63) / 64;
        if (!words || len != nc * b->H) return fail(GOL_ERR_INVALID, "words length must be height * ceil(width/64)");
        if (b->multi) return b->multi->save_packed(words);
        GOL_RC(sync_bytes(b));
        const size_t n = (size_t)len * 8;
        DeviceBuffer staging;
        GOL_RC(staging.alloc(n, "snapshot"));
        GOL_HIP(gol::launch_export_canonical(b->buf[b->cur], b->W, b->H, b->pitch, 0, b->packed ? b->ilv : 0,
                                             staging.as<uint64_t>(), b->stream));
        GOL_HIP(hipMemcpyAsync(words, staging.p, n, hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return check_valid(b);
    });
}

int gol_load_packed(gol_board* b, const uint64_t* words, int64_t len) {
    return with_board(b, [&] {
        const int64_t nc = (b->W + 63) / 64;
        if (!words || len != nc * b->H) return fail(GOL_ERR_INVALID, "words length must be height * ceil(width/64)");
        b->generation = 0;
        if (b->multi) return b->multi->load_packed(words);
        const size_t n = (size_t)len * 8;
        DeviceBuffer staging;
        GOL_RC(staging.alloc(n, "snapshot"));
        GOL_HIP(hipMemcpyAsync(staging.p, words, n, hipMemcpyHostToDevice, b->stream));
        GOL_HIP(gol::launch_import_canonical(staging.as<uint64_t>(), b->W, b->H, b->pitch, 0, b->packed ? b->ilv : 0,
                                             b->buf[b->cur], b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return overwritten(b);
    });
}

int gol_seed_dotnet(gol_board* b, int32_t seed, int mode) {
    return with_board(b, [&] {
        if (mode != GOL_INIT_DOTNET_MOD2 && mode != GOL_INIT_DOTNET_NEXT2) return fail(GOL_ERR_INVALID, "bad mode");
        std::vector<uint8_t> cells((size_t)(b->W * b->H));
        gol::DotNetRandom r(seed);
        // creation order x outer, y inner (GameOfLifeDriver.fs:16-19; Array2D.init in Script.fsx:27)
        for (int64_t x = 0; x < b->W; x++)
            for (int64_t y = 0; y < b->H; y++)
                cells[(size_t)(x + y * b->W)] = (mode == GOL_INIT_DOTNET_MOD2) ? (r.Next() % 2 == 0) : (r.Next(2) == 0);
        b->generation = 0;
        return set_cells_impl(b, cells.data());
    });
}

int gol_seed_splitmix(gol_board* b, uint64_t seed) {
    return with_board(b, [&] {
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
    });
}

int gol_clear(gol_board* b) {
    return with_board(b, [&] {
        if (b->multi) {
            b->generation = 0;
            return b->multi->clear();
        }
        GOL_HIP(hipMemsetAsync(b->buf[b->cur], 0, b->bytes(), b->stream));
        b->generation = 0;
        return overwritten(b);
    });
}

int gol_place_rle(gol_board* b, const char* rle, int64_t x, int64_t y) {
    return with_board(b, [&] {
        std::vector<std::pair<int64_t, int64_t>> pts;
        std::string err;
        if (!gol::parse_rle(rle, pts, err)) return fail(GOL_ERR_INVALID, err);
        std::vector<int64_t> xy;
        xy.reserve(pts.size() * 2);
        for (auto& p : pts) {
            xy.push_back((((x + p.first) % b->W) + b->W) % b->W);
            xy.push_back((((y + p.second) % b->H) + b->H) % b->H);
        }
        return place_points(b, xy);
    });
}

int gol_generation(gol_board* b, int64_t* out) {
    if (!b || !out) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    *out = b->generation;
    return GOL_OK;
}

int gol_synchronize(gol_board* b) {
    return with_board(b, [&] { return sync(b); });
}

int gol_population(gol_board* b, int64_t* out) {
    return with_board(b, [&] {
        if (!out) return fail(GOL_ERR_INVALID, "null out");
        uint64_t v = 0;
        GOL_RC(reduce_impl(b, false, &v));
        *out = (int64_t)v;
        return GOL_OK;
    });
}

int gol_hash(gol_board* b, uint64_t* out) {
    return with_board(b, [&] {
        if (!out) return fail(GOL_ERR_INVALID, "null out");
        return reduce_impl(b, true, out);
    });
}

// The board's rule (gol.h).  A property of the handle: nothing that writes cells touches it.
int gol_set_rule(gol_board* b, int birth, int survive) {
    return with_board(b, [&] {
        if (!gol::rule_masks_ok(birth, survive))
            return fail(GOL_ERR_INVALID, "rule: birth and survive masks must lie in 0..0x1FF");
        const uint32_t rule = gol::rule_pack(birth, survive);
        if (b->multi && rule != gol::kRuleLifePacked)
            return fail(GOL_ERR_UNSUPPORTED, "rule: a board on several GPUs runs B3/S23 only (its strip passes are the "
                                             "B3/S23 streaming kernels); the rule is unchanged");
        // the scratch rows of one rule's passes are not another's (B3/S23's may be ring or cooperative rows): the bytes
        // are the state from here on
        if (!b->multi) GOL_RC(sync_bytes(b));
        b->rule = rule;
        return GOL_OK;
    });
}

int gol_rule(gol_board* b, int* birth, int* survive) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    if (!birth || !survive) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    *birth = (int)(b->rule & gol::kRuleMaskMax);
    *survive = (int)(b->rule >> 9);
    return GOL_OK;
}

// A Generations rule on the board (gol.h): the rule and the states per cell.  The alive plane never moves; the decay
// buffers come and go with nstates.
int gol_set_generations_rule(gol_board* b, int birth, int survive, int nstates) {
    return with_board(b, [&] {
        if (!gol::rule_masks_ok(birth, survive))
            return fail(GOL_ERR_INVALID, "rule: birth and survive masks must lie in 0..0x1FF");
        if (!gol::gen_states_ok(nstates)) return fail(GOL_ERR_INVALID, "rule: nstates must be 2..8");
        const uint32_t rule = gol::rule_pack(birth, survive);
        if (b->multi && (nstates != 2 || rule != gol::kRuleLifePacked))
            return fail(GOL_ERR_UNSUPPORTED, "rule: a board on several GPUs runs B3/S23 at two states only (its strip "
                                             "passes are the B3/S23 streaming kernels); the rule is unchanged");
        if (b->multi) return GOL_OK;
        GOL_RC(sync_bytes(b));  // as gol_set_rule: the bytes are the state from here on
        if (nstates != b->nstates) {
            // every dying cell becomes dead: fresh zeroed buffers where the size changes, the old ones zeroed where
            // it does not; nothing of the board changes before every allocation has succeeded
            const size_t need = gol_board::dec_bytes_of(b, nstates);
            void* fresh[2] = {nullptr, nullptr};
            const bool realloc = need != b->dec_bytes();
            GOL_HIP(hipStreamSynchronize(b->stream));
            if (realloc && need) {
                for (void*& p : fresh) {
                    const hipError_t e = hipMalloc(&p, need);
                    if (e != hipSuccess) {
                        p = nullptr;
                        if (fresh[0]) (void)hipFree(fresh[0]);
                        return fail(GOL_ERR_OOM, std::string("hipMalloc decay planes: ") + hipGetErrorString(e));
                    }
                }
            }
            if (realloc) {
                for (int i = 0; i < 2; i++) {
                    if (b->dec[i]) (void)hipFree(b->dec[i]);
                    b->dec[i] = fresh[i];
                }
            }
            b->nstates = nstates;
            for (void* p : b->dec)
                if (p) GOL_HIP(hipMemsetAsync(p, 0, need, b->stream));
            GOL_HIP(hipStreamSynchronize(b->stream));
        }
        b->rule = rule;
        return GOL_OK;
    });
}

int gol_generations_rule(gol_board* b, int* birth, int* survive, int* nstates) {
    if (!b) return fail(GOL_ERR_INVALID, "null board");
    if (!birth || !survive || !nstates) return fail(GOL_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(b->mu);
    *birth = (int)(b->rule & gol::kRuleMaskMax);
    *survive = (int)(b->rule >> 9);
    *nstates = b->nstates;
    return GOL_OK;
}

int gol_set_states(gol_board* b, const uint8_t* states, int64_t len) {
    return with_board(b, [&] {
        if (!states || len != b->W * b->H) return fail(GOL_ERR_INVALID, "states length must be width*height");
        for (int64_t i = 0; i < len; i++)
            if (states[i] >= b->nstates) return fail(GOL_ERR_INVALID, "states: a byte is not below the board's nstates");
        b->generation = 0;  // a new board, as after every other setter (gol.h)
        if (b->multi) return set_cells_impl(b, states);  // two states: a state byte is a cell byte
        const size_t n = (size_t)len;
        DeviceBuffer staging;
        GOL_RC(staging.alloc(n));
        GOL_HIP(hipMemcpyAsync(staging.p, states, n, hipMemcpyHostToDevice, b->stream));
        GOL_HIP(gol::launch_states_pack(staging.as<uint8_t>(), b->buf[b->cur], b->dec[b->cur], b->packed ? b->ilv : 0,
                                        b->W, b->H, b->pitch, b->nstates, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return overwritten(b, false);
    });
}

int gol_get_states(gol_board* b, uint8_t* states, int64_t len) {
    return with_board(b, [&] {
        if (!states || len != b->W * b->H) return fail(GOL_ERR_INVALID, "states length must be width*height");
        if (b->multi) return readback_impl(b, states, b->W, 1);
        GOL_RC(sync_bytes(b));
        const size_t n = (size_t)len;
        DeviceBuffer staging;
        GOL_RC(staging.alloc(n));
        GOL_HIP(gol::launch_states_unpack(b->buf[b->cur], b->dec[b->cur], staging.as<uint8_t>(), b->packed ? b->ilv : 0,
                                          b->W, b->H, b->pitch, b->nstates, b->stream));
        GOL_HIP(hipMemcpyAsync(states, staging.p, n, hipMemcpyDeviceToHost, b->stream));
        GOL_HIP(hipStreamSynchronize(b->stream));
        return check_valid(b);
    });
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

}  // extern "C"
