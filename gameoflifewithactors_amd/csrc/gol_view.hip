// gol_view.hip -- zoomable density view of a board: live-cell counts of scale x scale pixels, and their Gray8 tone map.
//
// A view (x0, y0, s, out_w, out_h) covers the cells (x0 + s i + a, y0 + s j + b), 0 <= a, b < s, of pixel (i, j)
// (include/gol/gol.h gol_view_counts).  The host cuts it into the non-wrapping rectangles of one
// buffer (up to four on a torus, clipped to the board when bounded and to a strip's owned rows), and EVERY launch
// ADDS into the count buffer: rectangles, tiles cut by a seam or a strip boundary, and the row bands one tile row is
// split into all land in the same pixel by atomicAdd.
//
//   gol_view_pixels   any scale, packed or byte boards: one thread (s < 32) or one wave per (pixel, row band); the cells
//                     of a pixel inside one stored word are one contiguous bit range in every layout (gol_layout.h: bit
//                     b of word j is cell 32 M k + j + M b, monotonic in b), so the inner step is popc(word & mask).
//   gol_view_stream   wide tiles of packed boards, the zoomed-out hot path: lanes take consecutive words of a row
//                     (16-byte loads where the rows allow), loop down the rows of a band of ONE tile row, and count
//                     each word into at most T tiles through T masks hoisted out of the row loop (a word spans
//                     31 M + 1 cells: T = 2 for s >= 32 M, T = 3 for 16 M <= s < 32 M -- s = 64 at ilv 4); the
//                     workgroup's lanes are combined per tile in LDS, then one global atomicAdd per (workgroup, tile)
//                     (gol_formats.hip block_add records what per-wave device-scope atomics cost).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_internal.h"
#include "gol_layout.h"
#include "gol_view.h"

namespace gol {

namespace {

// One non-wrapping rectangle of a view inside one buffer.
struct ViewRect {
    const void* base;  // buffer row 0
    int64_t pitch;     // words (packed) or cells (bytes) per buffer row
    int64_t cx0, cx1;  // board columns [cx0, cx1)
    int64_t ry0, ry1;  // buffer rows [ry0, ry1)
    int64_t dx, dy;    // view cell (u, v) = (column + dx, buffer row + dy) >= 0; pixel (u / s, v / s)
    int64_t s, out_w;
    uint32_t* counts;
};

constexpr int kViewThreads = 256;
constexpr int kViewStreamMin = 16;  // gol_view_stream takes s >= 16 M: a word (31 M + 1 cells) then meets <= 3 tiles
constexpr int kViewTiles = 2056;  // tiles one workgroup of gol_view_stream can touch: 32768 cells / (s >= 16), + 3

__device__ __forceinline__ uint32_t bit_range(int lo, int hi) {  // bits [lo, hi), 0 <= lo <= hi <= 32
    if (hi <= lo) return 0u;
    const uint32_t upto = hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u);
    return upto & ~((1u << lo) - 1u);
}

__device__ __forceinline__ int clamp_bit(int64_t v, int lo, int hi) {
    return v < lo ? lo : (v > hi ? hi : (int)v);
}

// bits of stored word w (layout of shift sh, M = 1 << sh) whose cells lie in [xa, xb)
__device__ __forceinline__ uint32_t word_mask(int64_t w, int sh, int64_t xa, int64_t xb) {
    const int64_t M = (int64_t)1 << sh;
    const int64_t first = ((w >> sh) << (5 + sh)) + (w & (M - 1));  // cell of bit 0
    const int lo = clamp_bit((xa - first + M - 1) >> sh, 0, 32);     // ceil((xa - first) / M)
    const int hi = clamp_bit((xb - first + M - 1) >> sh, 0, 32);
    return bit_range(lo, hi);
}

// ------------------------------------------------------------------------------------------------
// Per-pixel kernel.  G lanes per unit (1 or 64); a unit is (pixel of the rectangle, row band blockIdx.y).  npx pixels
// across, npy_max pixel rows per band at most.
template <int G>
__global__ __launch_bounds__(kViewThreads) void gol_view_pixels(ViewRect r, int ilv, int64_t band_rows, int64_t npx,
                                                                int64_t npy_max) {
    const int64_t unit = ((int64_t)blockIdx.x * kViewThreads + threadIdx.x) / G;  // wave-uniform for G = 64
    const int lane = (int)(threadIdx.x % G);
    if (unit >= npx * npy_max) return;
    const int64_t rb0 = r.ry0 + (int64_t)blockIdx.y * band_rows;
    const int64_t rb1 = rb0 + band_rows < r.ry1 ? rb0 + band_rows : r.ry1;
    const int64_t i = (r.cx0 + r.dx) / r.s + unit % npx;
    const int64_t j = (rb0 + r.dy) / r.s + unit / npx;
    const int64_t ya = std::max(rb0, j * r.s - r.dy), yb = std::min(rb1, (j + 1) * r.s - r.dy);
    const int64_t xa = std::max(r.cx0, i * r.s - r.dx), xb = std::min(r.cx1, (i + 1) * r.s - r.dx);
    if (ya >= yb || xa >= xb) return;
    const int sh = ilv_shift(ilv);
    // items of one row: the stored words that hold cells of [xa, xb), or the cells themselves on a byte board
    const int64_t it0 = ilv ? ((xa >> (5 + sh)) << sh) : xa;
    const int64_t it1 = ilv ? ((((xb - 1) >> (5 + sh)) + 1) << sh) : xb;
    const int64_t n = it1 - it0;
    int across = 1;  // lanes across a row (a power of two), the others down the rows
    if (G > 1)
        while (across < G && across < n) across <<= 1;
    const int lr = lane / across, lc = lane % across, rstep = G / across;
    uint32_t sum = 0;
    for (int64_t y = ya + lr; y < yb; y += rstep) {
        if (ilv) {
            const uint32_t* row = static_cast<const uint32_t*>(r.base) + y * r.pitch;
            for (int64_t w = it0 + lc; w < it1; w += across) sum += __popc(row[w] & word_mask(w, sh, xa, xb));
        } else {
            const uint8_t* row = static_cast<const uint8_t*>(r.base) + y * r.pitch;
            for (int64_t x = it0 + lc; x < it1; x += across) sum += row[x] != 0;
        }
    }
    if (G > 1) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
        if (lane != 0) return;
    }
    if (sum) atomicAdd(r.counts + j * r.out_w + i, sum);
}

// ------------------------------------------------------------------------------------------------
// Streaming kernel for wide tiles.  A workgroup takes (chunk of 2^lx_log2 * VEC consecutive words, band of one tile
// row); its lanes are 2^lx_log2 across and 256 >> lx_log2 down.  Words [w_first, w_end) hold the rectangle's columns
// (w_first a multiple of VEC).  Tile rows are cut into nb bands of band_rows rows each.
template <int ILV, int VEC, int T>
__global__ __launch_bounds__(kViewThreads) void gol_view_stream(ViewRect r, int lx_log2, int64_t nchunks, int nb,
                                                                int64_t band_rows, int64_t w_first, int64_t w_end) {
    __shared__ uint32_t tiles[kViewTiles];
    constexpr int sh = ILV == 4 ? 2 : (ILV == 2 ? 1 : 0);
    const int lanes_x = 1 << lx_log2, lanes_y = kViewThreads >> lx_log2;
    const int lx = (int)threadIdx.x & (lanes_x - 1), ly = (int)threadIdx.x >> lx_log2;
    int64_t bid = blockIdx.x;
    const int64_t chunk = bid % nchunks;
    bid /= nchunks;
    const int band = (int)(bid % nb);
    const int64_t j = (r.ry0 + r.dy) / r.s + bid / nb;  // the band's tile row
    const int64_t ya = std::max(r.ry0, j * r.s - r.dy) + band * band_rows;
    const int64_t yb = std::min(std::min(r.ry1, (j + 1) * r.s - r.dy), ya + band_rows);
    // the chunk's words and the rectangle's cells they can hold (whole blocks: a lower / upper bound)
    const int64_t cw0 = w_first + chunk * ((int64_t)lanes_x * VEC);
    const int64_t cw1 = std::min(w_end, cw0 + (int64_t)lanes_x * VEC);
    const int64_t cell0 = std::max(r.cx0, (cw0 >> sh) << (5 + sh));
    const int64_t cell1 = std::min(r.cx1, (((cw1 - 1) >> sh) + 1) << (5 + sh));
    if (ya >= yb || cell0 >= cell1) return;  // uniform over the workgroup
    const int64_t tile_first = (cell0 + r.dx) / r.s;
    const int ntl = (int)std::min<int64_t>((cell1 - 1 + r.dx) / r.s - tile_first + 1, kViewTiles);
    for (int k = threadIdx.x; k < ntl; k += kViewThreads) tiles[k] = 0;

    // Per word: m[k] = its bits inside the rectangle that lie in its first k + 1 tiles (m[T - 1]: all of them).  A word
    // spans 31 M + 1 cells, so it meets at most T - 1 tile boundaries, at positions that depend on the column only.
    uint32_t m[VEC][T], c[VEC][T];
    int t_lo[VEC];
    const int64_t w0 = cw0 + (int64_t)lx * VEC;
#pragma unroll
    for (int v = 0; v < VEC; v++) {
#pragma unroll
        for (int k = 0; k < T; k++) m[v][k] = c[v][k] = 0;
        t_lo[v] = 0;
        const int64_t w = w0 + v;
        if (w >= cw1) continue;
        const int64_t first = ((w >> sh) << (5 + sh)) + (w & (ILV - 1));
        const int lo = clamp_bit((r.cx0 - first + ILV - 1) >> sh, 0, 32);
        const int hi = clamp_bit((r.cx1 - first + ILV - 1) >> sh, 0, 32);
        if (hi <= lo) continue;
        const int64_t t = (first + ((int64_t)lo << sh) + r.dx) / r.s;
#pragma unroll
        for (int k = 0; k < T - 1; k++)  // bits below the first cell of tile t + k + 1
            m[v][k] = bit_range(lo, clamp_bit(((t + k + 1) * r.s - r.dx - first + ILV - 1) >> sh, lo, hi));
        m[v][T - 1] = bit_range(lo, hi);
        t_lo[v] = (int)std::min<int64_t>(t - tile_first, kViewTiles - T);
    }
    if (w0 < cw1) {
        constexpr int kInFlight = T == 2 ? 4 : 2;
        const int64_t step = (int64_t)lanes_y * r.pitch;  // 64-bit row offsets: strip buffers pass 4 GiB
        const uint32_t* p = static_cast<const uint32_t*>(r.base) + (ya + ly) * r.pitch + w0;
        // rows in flight per lane: 4 with two masks per word, 2 with three (64 VGPRs: 8 waves per SIMD either way)
#pragma unroll kInFlight
        for (int64_t y = ya + ly; y < yb; y += lanes_y, p += step) {
            uint32_t x[VEC];
            if constexpr (VEC == 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(p);  // global_load_dwordx4: 1 KiB per wave and row
                x[0] = q.x;
                x[1] = q.y;
                x[2] = q.z;
                x[3] = q.w;
            } else {
                x[0] = *p;
            }
#pragma unroll
            for (int v = 0; v < VEC; v++)
#pragma unroll
                for (int k = 0; k < T; k++) c[v][k] += __popc(x[v] & m[v][k]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        uint32_t below = 0;
#pragma unroll
        for (int k = 0; k < T; k++) {  // the counts are cumulative over the word's tiles
            if (c[v][k] != below) atomicAdd(&tiles[t_lo[v] + k], c[v][k] - below);
            below = c[v][k];
        }
    }
    __syncthreads();
    uint32_t* out = r.counts + j * r.out_w + tile_first;
    for (int k = threadIdx.x; k < ntl; k += kViewThreads)
        if (tiles[k]) atomicAdd(out + k, tiles[k]);
}

__global__ __launch_bounds__(kViewThreads) void gol_view_tone_map(const uint32_t* __restrict__ counts,
                                                                  uint8_t* __restrict__ pixels, int64_t out_w,
                                                                  int64_t out_h, int64_t stride, int64_t scale, int mode,
                                                                  uint8_t alive_value) {
    const int64_t idx = (int64_t)blockIdx.x * kViewThreads + threadIdx.x;
    if (idx >= out_w * out_h) return;
    pixels[idx % out_w + idx / out_w * stride] = view_tone(counts[idx], scale, mode, alive_value);
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workgroups the reductions aim for: 8 per CU (256 CUs without a device query)
int64_t target_groups() {
    const int cus = device_cus();
    return (int64_t)(cus > 0 ? cus : 256) * 8;
}

hipError_t launch_pixels(const ViewRect& r, int ilv, hipStream_t s) {
    const int64_t npx = (r.cx1 - 1 + r.dx) / r.s - (r.cx0 + r.dx) / r.s + 1;
    const int64_t npy = (r.ry1 - 1 + r.dy) / r.s - (r.ry0 + r.dy) / r.s + 1;
    const int64_t rows = r.ry1 - r.ry0;
    const int G = r.s >= 32 ? 64 : 1;
    int64_t nbands = 1;
    if (G > 1) {  // few large pixels: cut the rows into bands until the waves fill the device
        nbands = ceil_div(target_groups() * (kViewThreads / 64), npx * npy);
        nbands = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nbands, ceil_div(rows, 16)), 65535));
    }
    const int64_t band_rows = ceil_div(rows, nbands);
    nbands = ceil_div(rows, band_rows);
    const int64_t npy_max = std::min(npy, (band_rows + r.s - 2) / r.s + 1);
    const int64_t grid = ceil_div(npx * npy_max * G, kViewThreads);
    if (grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (G > 1)
        hipLaunchKernelGGL((gol_view_pixels<64>), dim3((unsigned)grid, (unsigned)nbands), dim3(kViewThreads), 0, s, r, ilv,
                           band_rows, npx, npy_max);
    else
        hipLaunchKernelGGL((gol_view_pixels<1>), dim3((unsigned)grid, (unsigned)nbands), dim3(kViewThreads), 0, s, r, ilv,
                           band_rows, npx, npy_max);
    return hipGetLastError();
}

template <int ILV, int VEC, int T>
hipError_t launch_stream_t(const ViewRect& r, hipStream_t s, bool* taken) {
    constexpr int sh = ILV == 4 ? 2 : (ILV == 2 ? 1 : 0);
    const int64_t w_first = ((r.cx0 >> (5 + sh)) << sh) / VEC * VEC;
    const int64_t w_end = (((r.cx1 - 1) >> (5 + sh)) + 1) << sh;
    const int64_t ngroups = ceil_div(w_end - w_first, VEC);
    int lx_log2 = 0;
    while ((1 << lx_log2) < kViewThreads && (1 << lx_log2) < ngroups) lx_log2++;
    const int64_t lanes_x = (int64_t)1 << lx_log2, lanes_y = kViewThreads / lanes_x;
    const int64_t nchunks = ceil_div(ngroups, lanes_x);
    const int64_t ntr = (r.ry1 - 1 + r.dy) / r.s - (r.ry0 + r.dy) / r.s + 1;
    // Parallelism comes from the input: a tile row is cut into bands (of at least 4 rows per lane) until the grid
    // fills the device, whatever the number of output pixels.
    int64_t nb = ceil_div(target_groups(), nchunks * ntr);
    nb = std::max<int64_t>(1, std::min(nb, r.s / (lanes_y * 4)));
    const int64_t band_rows = ceil_div(r.s, nb);
    nb = ceil_div(r.s, band_rows);
    const int64_t grid = nchunks * ntr * nb;
    if (grid >= ((int64_t)1 << 31)) return hipSuccess;  // not taken: the per-pixel kernel does it
    *taken = true;
    hipLaunchKernelGGL((gol_view_stream<ILV, VEC, T>), dim3((unsigned)grid), dim3(kViewThreads), 0, s, r, lx_log2, nchunks,
                       (int)nb, band_rows, w_first, w_end);
    return hipGetLastError();
}

template <int ILV>
hipError_t launch_stream_ilv(const ViewRect& r, hipStream_t s, bool* taken) {
    // 16-byte loads need 16-byte rows; any other pitch or base streams with dword loads
    const bool vec4 = r.pitch % 4 == 0 && reinterpret_cast<uintptr_t>(r.base) % 16 == 0;
    if (r.s >= 32 * ILV)  // a word meets at most one tile boundary
        return vec4 ? launch_stream_t<ILV, 4, 2>(r, s, taken) : launch_stream_t<ILV, 1, 2>(r, s, taken);
    return vec4 ? launch_stream_t<ILV, 4, 3>(r, s, taken) : launch_stream_t<ILV, 1, 3>(r, s, taken);
}

hipError_t launch_stream(const ViewRect& r, int ilv, hipStream_t s, bool* taken) {
    if (ilv == 1) return launch_stream_ilv<1>(r, s, taken);
    if (ilv == 2) return launch_stream_ilv<2>(r, s, taken);
    return launch_stream_ilv<4>(r, s, taken);
}

// [begin, end) of board coordinates and the offset d with view coordinate = board coordinate + d
struct Span {
    int64_t begin, end, d;
};

// the (at most two) non-wrapping spans of view coordinates [0, n) starting at board coordinate o, on an axis of size
int spans(int64_t o, int64_t n, int64_t size, bool torus, Span out[2]) {
    int k = 0;
    if (torus) {  // 0 <= o < size, n <= size
        out[k++] = Span{o, std::min(size, o + n), -o};
        if (o + n > size) out[k++] = Span{0, o + n - size, size - o};
    } else {
        const int64_t b = std::max<int64_t>(0, o), e = std::min(size, o + n);
        if (b < e) out[k++] = Span{b, e, -o};
    }
    return k;
}

}  // namespace

hipError_t launch_view_counts(const ViewSource& src, const ViewArgs& v, uint32_t* counts, bool stream_kernel,
                              hipStream_t s) {
    Span xs[2], ys[2];
    const int nx = spans(v.x, v.s * v.out_w, src.W, src.torus, xs);
    const int ny = spans(v.y, v.s * v.out_h, src.H, src.torus, ys);
    for (int a = 0; a < ny; a++) {
        // the span's rows this buffer owns
        const int64_t g0 = std::max(ys[a].begin, src.y0), g1 = std::min(ys[a].end, src.y0 + src.rows);
        if (g0 >= g1) continue;
        for (int b = 0; b < nx; b++) {
            ViewRect r;
            r.base = src.base;
            r.pitch = src.pitch;
            r.cx0 = xs[b].begin;
            r.cx1 = xs[b].end;
            r.ry0 = g0 - src.y0 + src.row0;
            r.ry1 = g1 - src.y0 + src.row0;
            r.dx = xs[b].d;
            r.dy = ys[a].d + src.y0 - src.row0;
            r.s = v.s;
            r.out_w = v.out_w;
            r.counts = counts;
            bool taken = false;
            if (stream_kernel && src.ilv > 0 && v.s >= kViewStreamMin * src.ilv)
                if (hipError_t e = launch_stream(r, src.ilv, s, &taken)) return e;
            if (!taken)
                if (hipError_t e = launch_pixels(r, src.ilv, s)) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_view_tone(const uint32_t* counts, uint8_t* pixels, int64_t out_w, int64_t out_h, int64_t stride,
                            int64_t scale, int mode, uint8_t alive_value, hipStream_t s) {
    hipLaunchKernelGGL(gol_view_tone_map, dim3((unsigned)ceil_div(out_w * out_h, kViewThreads)), dim3(kViewThreads), 0, s,
                       counts, pixels, out_w, out_h, stride, scale, mode, alive_value);
    return hipGetLastError();
}

}  // namespace gol
