// gol_strip.cpp -- the row-strip primitives of the C ABI (include/gol/gol.h gol_strip_*: what a multi-GPU driver, or
// the multi board of gol_multi.cpp, runs on one strip of a board) and the level-pipelined pass's debug entry points
// (gol_debug.h).  They take no board handle: geometry is checked on the host, then one launch on the caller's stream.
#include <algorithm>

#include "gol_board.h"
#include "gol_debug.h"
#include "gol_view.h"

using gol::fail;

namespace {

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
    // a lane moves its block (ilv words) as one 4 * ilv-byte load, store or LDS-DMA: rows start on that boundary when
    // the buffers do (the pitch is a multiple of ilv)
    const uintptr_t block_bytes = 4 * (uintptr_t)s->ilv;
    if ((uintptr_t)src % block_bytes || (uintptr_t)dst % block_bytes)
        return fail(GOL_ERR_INVALID, "src and dst must be aligned to 4 * ilv bytes");
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
