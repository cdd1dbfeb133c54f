/*
 * gol.h -- C ABI of the MI355X Game of Life engine (libgol_hip.so).
 *
 * Drop-in boundary for the reference's hot path: the per-cell actors of
 *   GameOfLife/GameOfLife/GameOfLifeLogic.fs:39-71   (MailboxProcessor cell, `createCell`)
 *   GameOfLife/GameOfLifeAkka/GameofLife.fs:88-138   (Akka `CellAkka`, `ICell.Send`)
 * and the dictionary of them built by the driver (GameOfLifeDriver.fs:16-30, GameofLife.fs:148-163).
 * One board handle replaces the W*H cell actors; `gol_step(b, 1)` replaces one `updateView()` tick
 * (GameOfLifeDriver.fs:32-34); `gol_render_gray8` / `gol_get_cells` replace the W*H `Update` posts
 * consumed by the render agent (GameOfLifeUI.fs:21-31).  The F# P/Invoke declarations that bind each
 * entry point are in INTEGRATION.md.
 *
 * Conventions: cdecl, plain pointers, int64_t sizes.  Every function returns 0 (GOL_OK) or a negative
 * GOL_ERR_* code; gol_last_error() returns a thread-local message for the last failure on the calling
 * thread.  No C++ exception crosses this ABI.  Host buffers are borrowed for the duration of the call
 * only (P/Invoke pins blittable byte[] for the call).  Each board handle is serialised by an internal
 * mutex (the reference's timer can re-enter updateView, GameOfLifeDriver.fs:38-40); separate handles are
 * independent.  Cell layout for host buffers: one byte per cell, index x + y*width, nonzero = alive
 * (GameOfLifeUI.fs:24-28 pixel order).
 */
#ifndef GOL_GOL_H
#define GOL_GOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOL_OK 0
#define GOL_ERR_INVALID -1     /* bad argument, size or geometry */
#define GOL_ERR_HIP -2         /* HIP runtime / kernel launch failure */
#define GOL_ERR_OOM -3         /* device allocation failed */
#define GOL_ERR_UNSUPPORTED -4 /* valid request this build does not implement */
#define GOL_ERR_NO_DEVICE -5   /* no usable gfx950 device */

enum { GOL_TORUS = 0, GOL_BOUNDED = 1 };
/* gol_seed_dotnet modes */
enum {
    GOL_INIT_DOTNET_MOD2 = 0, /* GameOfLifeDriver.fs:9-11,16-19: x outer, y inner, Random.Next() % 2 = 0 */
    GOL_INIT_DOTNET_NEXT2 = 1 /* Script.fsx:25-27: Array2D.init (x outer), Random.Next 2 = 0 */
};

typedef struct gol_board gol_board; /* opaque; library-owned */

/* Replaces `cells = seq { for x .. for y .. createCell ... } |> dict` (GameOfLifeDriver.fs:16-19) and the
 * neighbour wiring (L21-30).  width/height >= 3 (smaller tori alias neighbours: the reference's
 * Dictionary never reaches 8 keys and the board freezes, GameOfLifeLogic.fs:58 -- rejected here).
 * boundary: GOL_TORUS (actors, GameOfLifeDriver.fs:25) or GOL_BOUNDED (Script.fsx:11).
 * num_gpus: 1 = one board on the calling thread's current device.  N > 1 = row strips on devices
 *           0..N-1 of THIS process (the reference host is one process, GameOfLifeDriver.fs:13-41): strip r
 *           owns rows [H*r/N, H*(r+1)/N); every pass moves k halo rows between neighbouring strips while the
 *           interior rows compute.  Halo transport: peer copies (hipMemcpyPeerAsync, xGMI between GPUs) by
 *           default; RCCL send/recv on request (gol_set_option "transport" = 2, distinct devices only;
 *           gol_transport reports which one runs).  Needs width % 32 == 0.  Bit-identical to num_gpus = 1.
 *           (One process per GPU instead: gol_strip_* below.)
 * tblock_k: upper bound on the generations fused per kernel pass (0 = the engine's default for the
 *           board, gol_layout / gol_info report it):
 *             packed boards below 2^25 cells: ilv 1, k = 8 (latency-bound: the single-wave pass takes boards up
 *               to 128 x 256), except single boards the cooperative pass takes (2^17 < cells <=
 *               2^26, 4096 or 8192 wide): ilv 2 / 4 (that pass's words per lane) and k = 16 / 8, of
 *               which it hands off every min(k, 8) generations;
 *             packed boards of 2^25 .. 2^29 cells, width % 64 == 0: ilv 2, k = 16;
 *             boards from 2^30 cells per part, width % 128 == 0 and >= 7936 (torus) or 8192 (bounded): ilv 4,
 *               k = 32 -- the level-pipelined pass (k = 16 / 32 at ilv 4 is that pass);
 *             other packed boards from 2^29 cells, width % 64 == 0: ilv 2, k = 12 -- torus and bounded alike
 *               (bounded boards ran k = 16 until round 3), single board or strips;
 *             other packed widths from 2^25 cells: ilv 1, k = 32;
 *             byte boards (width % 32 != 0, ilv 0) below 3 * 2^26 cells: k = 8 below 2^25 cells, 16 below 2^27,
 *               24 above (the ilv-1 scratch rows they stream as);
 *             byte boards from 3 * 2^26 cells: the rules above for the block rows they stream as (DESIGN.md 4.1
 *               "Ragged rows": 2 * ceil((W + 128) / 64) words per ring row on a torus, 2 * ceil(W / 64) when
 *               bounded; ilv 2 k = 16 below 2^29 of those cells, k = 12 above);
 *           else one of 1,2,4,6,8,12,16,24,32 -- the engine uses the deepest supported depth <= tblock_k (a
 *           depth the automatic ilv 4 does not run, 12 or 24, selects ilv 2 instead).
 *           A multi-part board's halo depth (gol_part_info ghost) is the deepest supported k <= tblock_k that
 *           fits its thinnest strip.
 * The initial board is all dead. */
int gol_create(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, gol_board** out);
/* As gol_create with an explicit packed layout: ilv = 0 (auto, gol_default_ilv) or 1, 2, 4 words per
 * interleaved block (width must be a multiple of 32*ilv). */
int gol_create_ex(int64_t width, int64_t height, int boundary, int num_gpus, int tblock_k, int ilv,
                  gol_board** out);
/* As gol_create_ex with num_gpus = ndevices and strip r placed on devices[r] (a device may repeat, e.g.
 * to run the multi-strip protocol on one GPU). */
int gol_create_multi(int64_t width, int64_t height, int boundary, const int* devices, int ndevices, int tblock_k,
                     int ilv, gol_board** out);
/* Row strips of a board (1 unless created with num_gpus > 1) and where strip `part` lives: its device,
 * first global row, owned rows and halo depth (ghost rows per side; 0 for a single board). */
int gol_num_parts(gol_board* b, int* n);
int gol_part_info(gol_board* b, int part, int* device, int64_t* y0, int64_t* rows, int64_t* ghost);
/* How a multi-part board moves its halo rows: peer copies (the default) or RCCL send/recv (ncclCommInitAll over
 * the parts' devices, xGMI) once gol_set_option(b, "transport", GOL_TRANSPORT_RCCL) succeeded -- it fails with
 * GOL_ERR_UNSUPPORTED when a device repeats (RCCL refuses two ranks on one GPU) or RCCL is unavailable, and the
 * board keeps peer copies.  A single board has none.  note (may be NULL, >= 256 bytes): a description. */
enum { GOL_TRANSPORT_NONE = 0, GOL_TRANSPORT_PEER = 1, GOL_TRANSPORT_RCCL = 2 };
int gol_transport(gol_board* b, int* transport, char* note, int64_t note_len);
int gol_destroy(gol_board* b);

/* Board I/O: cells[x + y*width], len == width*height.  Replaces createCell's `alive` argument
 * (GameOfLifeLogic.fs:39) and, on readback, the per-cell Update(alive, location) stream (L64).  gol_set_cells, like
 * every call that replaces the whole board (the seeds, gol_load_packed, gol_clear), resets the generation counter. */
int gol_set_cells(gol_board* b, const uint8_t* cells, int64_t len);
int gol_get_cells(gol_board* b, uint8_t* cells, int64_t len);
/* Read a window (x, y, w, h) of the board (no wrap; must lie inside): out[i + j*w] = cell (x+i, y+j). */
int gol_get_region(gol_board* b, int64_t x, int64_t y, int64_t w, int64_t h, uint8_t* out);

/* Seeding.  gol_seed_dotnet restates .NET Framework System.Random(seed) exactly as the reference uses it
 * (GameOfLifeDriver.fs:9-11 with an explicit seed instead of DateTime.Now.Ticks).  gol_seed_splitmix is
 * the build-owned device-side init for large boards.  gol_place_rle ORs a Life RLE pattern
 * with its top-left at (x, y), wrapped modulo the board. */
int gol_seed_dotnet(gol_board* b, int32_t seed, int mode);
/* Board snapshot (save / restore, SURVEY 8f "board save/load") in the canonical bit-packed layout the
 * hash is defined on, independent of the board's internal layout and GPU count: row y is ceil(width/64)
 * little-endian uint64 words, bit i of word j = cell (64j + i, y), bits past the width zero;
 * len = height * ceil(width/64).  A snapshot taken from any board loads into any board of the same size.
 * gol_load_packed resets the generation counter (like gol_set_cells). */
int gol_save_packed(gol_board* b, uint64_t* words, int64_t len);
int gol_load_packed(gol_board* b, const uint64_t* words, int64_t len);
int gol_seed_splitmix(gol_board* b, uint64_t seed);
int gol_place_rle(gol_board* b, const char* rle, int64_t x, int64_t y);
int gol_clear(gol_board* b);

/* Advance `generations` synchronous B3/S23 generations (GameOfLifeLogic.fs:47-66 under the Reset->State
 * phase barrier).  Asynchronous with respect to the host; any readback synchronises (and reports a failed
 * cooperative pass: the board is then invalid until overwritten).  Small and mid-size boards run the whole call
 * as one launch (single-wave, cooperative or LDS-resident pass: DESIGN.md 4.3-4.5; gol_set_option moves the
 * cut-overs); results are identical either way.  A board whose width is not a multiple of 32 runs calls of several
 * generations on whole-word scratch rows (DESIGN.md 4.1 "Ragged rows") and keeps its state there until another
 * call reads or replaces the cells. */
int gol_step(gol_board* b, int64_t generations);
int gol_generation(gol_board* b, int64_t* out);
int gol_synchronize(gol_board* b);
/* Profiling: gol_step between two HIP timing events on the board's stream, then synchronise; *elapsed_us = the
 * device time of the call (multi-part boards: each part times its own compute stream, the longest is reported).
 * Lets a host without any other GPU runtime (the F# driver) time the engine under the HIP runtime it loads. */
int gol_step_timed(gol_board* b, int64_t generations, double* elapsed_us);

/* Replaces the render agent's pixel fill (GameOfLifeUI.fs:24-28; GameofLife.fs:53-57; Script.fsx:33-35):
 * pixels[x + y*stride] = alive ? alive_value : 0, stride >= width, buffer >= stride*height bytes; the bytes between
 * width and stride of every row are set to 0 (all stride*height bytes are written, none beyond them). */
int gol_render_gray8(gol_board* b, uint8_t* pixels, int64_t stride, uint8_t alive_value);

/* A zoomable view of the board: what the render agent shows (GameOfLifeUI.fs:21-31) for boards no screen holds at one
 * byte per cell.  Pixel (i, j) of a view covers the scale x scale cells (x + scale*i + a, y + scale*j + b),
 * 0 <= a, b < scale; its count is the number of those cells that are alive.
 *   GOL_TORUS:   coordinates wrap modulo width / height; 0 <= x < width, 0 <= y < height, scale*out_w <= width and
 *                scale*out_h <= height (no cell is counted twice).
 *   GOL_BOUNDED: cells outside the board are dead; x and y may be anything in [-2^31, 2^31], so a view may overhang
 *                the board or lie wholly outside it.
 *   Limits:      1 <= scale <= 32768 (a count fits uint32), out_w, out_h >= 1, out_w*out_h <= 2^26; anything else
 *                returns GOL_ERR_INVALID before any device work.
 * A view reads the board once and changes neither the board, its generation nor its hash; only the
 * out_w*out_h counts (gol_view_counts) or out_h*stride bytes (gol_render_view) cross to the host.  Works on every
 * layout, on byte boards and on multi-part boards. */
typedef struct gol_view {
    int64_t x, y, scale, out_w, out_h;
} gol_view;
enum { GOL_VIEW_ANY = 0, GOL_VIEW_DENSITY = 1 };
/* counts[i + j*out_w] = live cells of pixel (i, j); host buffer of out_w*out_h uint32. */
int gol_view_counts(gol_board* b, const gol_view* v, uint32_t* counts);
/* pixels[i + j*stride] = gol_view_tone(count of pixel (i, j), scale, mode, alive_value); stride >= out_w, buffer >=
 * stride*out_h bytes, the bytes between out_w and stride are set to 0.  With scale 1, x = y = 0 and out_w x out_h =
 * width x height either mode gives the frame of gol_render_gray8. */
int gol_render_view(gol_board* b, const gol_view* v, int mode, uint8_t alive_value, uint8_t* pixels, int64_t stride);
/* Host-only, pure (like gol_hash_finalize): the Gray8 tone of a pixel of n = scale*scale cells.
 *   GOL_VIEW_ANY:     count ? alive_value : 0
 *   GOL_VIEW_DENSITY: (2*count*alive_value + n) / (2*n) in 64-bit integers (round half up)
 * 0 for any other mode or a scale outside 1..32768. */
uint8_t gol_view_tone(uint32_t count, int64_t scale, int mode, uint8_t alive_value);

/* Observables for parity checks. */
int gol_population(gol_board* b, int64_t* out);
int gol_hash(gol_board* b, uint64_t* out); /* canonical 64-bit board hash */

/* Introspection: width, height, boundary, tblock_k, packed (1 = bit-packed path, 0 = byte path). */
int gol_info(gol_board* b, int64_t* width, int64_t* height, int* boundary, int* tblock_k, int* packed);
/* Packed layout of the board: ilv = words per interleaved block (1, 2, 4; 0 = byte board), pitch in words. */
int gol_layout(gol_board* b, int* ilv, int64_t* pitch);
/* Layout / depth the engine picks for a large board of this width (0 if the width is not a multiple of
 * 32; boards below 2^25 cells use ilv 1, see gol_create), the default temporal-block depth for a layout
 * on a large board, and whether the step kernel supports depth k for a layout. */
int gol_default_ilv(int64_t width);
/* HIP devices visible to this process (0 and GOL_OK when there is none). */
int gol_device_count(int* n);
int gol_default_tblock(int ilv);
int gol_supported_k(int k, int ilv);
/* The layout and depth the engine picks for a board or row strip of `rows` rows (gol_create uses the same rule):
 * boards of >= 2^30 cells at least 7936 cells wide on a torus, 8192 bounded (width % 128 == 0) run the
 * level-pipelined pass, ilv 4 and K = 32; others as gol_default_ilv / gol_default_tblock.  k = 16 / 32
 * at ilv 4 is that pass (gol_strip_step refuses it on narrower strips). */
int gol_default_layout(int64_t width, int64_t rows, int boundary, int* ilv, int* tblock_k);
/* The HIP stream the board's kernels run on (hipStream_t), for event timing by a caller (multi-GPU
 * boards: strip 0's compute stream, which every pass joins at its end). */
int gol_stream(gol_board* b, void** stream);

/* Profiling: advance the board by ONE pass of its temporal depth with HIP timing events and report, per
 * row strip (n = gol_num_parts), the microseconds from the pass start to the end of the interior launch
 * (interior_us), to the release of the edge-band stream once the neighbours' halo rows have landed
 * (wait_us: the edge-band wait) and to the end of the edge bands (edge_us).  A single board times one
 * streaming pass and reports it in interior_us and edge_us and 0 in wait_us; a single board whose gol_step
 * runs another pass (single-wave, cooperative, LDS-resident) returns GOL_ERR_UNSUPPORTED.  Counts toward
 * gol_generation. */
int gol_pass_timing(gol_board* b, int n, double* interior_us, double* wait_us, double* edge_us);

/* Per-board path and tuning options (the library reads no environment variable).  Names, defaults first:
 *   "coop" 1 | 0                 cooperative register-band pass for mid-size boards
 *   "coop_k" 0 | 1..64           generations per band hand-off (0: min(tblock_k, 8))
 *   "coop_max_cells" 2^26        largest board that pass takes
 *   "resident_max_cells" -1 | n  LDS-resident pass cut-over (-1: 2^17 packed cells, off for byte boards; 0: off)
 *   "wave_resident" 1 | 0        single-wave pass for boards up to 128 x 256
 *   "split" 0 | n | -1           streaming pass: the oldest wave's share of a SIMD group segment in 1/65536
 *                                (0: the measured default, -1: no split)
 *   "split2" 0 | n               streaming pass, three waves per SIMD group: the middle wave's share of the two
 *                                younger waves' rows in 1/65536 (0: the measured default)
 *   "seg_rows" 0 | n             streaming pass: rows per wave segment (0: planned)
 *   "seam" 0 | -1                streaming pass on a torus: seam strips where they apply (-1: halo-lane strips)
 *   "transport" 1 | 2            multi-part boards: halo rows by peer copies (1) or RCCL (2, distinct devices;
 *                                GOL_ERR_UNSUPPORTED otherwise); GOL_ERR_UNSUPPORTED on a single board
 *   ("split", "split2", "seg_rows" and "seam" apply to every strip launch of a multi-part board as well)
 *   "ragged_ring" 1 | 2 | 0      ragged boards on the streaming pass as block rows in the aligned layouts (torus: ring
 *                                rows; bounded: column-masked rows) from 3 * 2^26 cells (1), on every size (2), or
 *                                never (0: ilv-1 rows)
 *   "ragged_stream" 1 | 0        boards of any width beyond the cooperative pass: the streaming pass on scratch
 *                                words (0: the per-generation byte step)
 *   "coop_poll_delay" -1 | 0..4096  s_sleep periods before a hand-off's first poll (-1: on the cooperative pass 0 for
 *                                4096-cell rows, 4 for narrower ones, 24 for every width above 4096; 8 on the rows-on-lanes pass)
 *   "lanes" 2 | 1 | 0            rows-on-lanes band pass in place of the cooperative one (packed single boards whose
 *                                width splits into 128/256/512/1024-column windows, coop_k <= 10, calls of >= 2 k
 *                                generations, every band resident at once): 2 = on the sizes it
 *                                measured faster (rows of <= 1024 cells), 1 = wherever it
 *                                applies, 0 = never
 *   "lanes_m" 0 | 3 | 5 | 9 | 17 its words per lane and half-row (0: 3 up to 1024 columns, else 9 when W % 512 == 0)
 *   "view_stream" 1 | 0          views (gol_view_counts / gol_render_view) of packed boards with scale >= 16 * ilv on the
 *                                streaming kernel (0: every view on the per-pixel kernel, the library's cross-check)
 *   "rule_ragged" 1 | 2 | 0      ragged boards (width not a multiple of 32, at least 64) under another rule, life-like or
 *                                Generations: the streaming passes on whole-word scratch rows in place of the
 *                                per-generation byte step -- on boards of more than 128 x 256 cells
 *                                (Generations rules: 2^22 cells) and calls of at least 4 generations (1), on every
 *                                such board and call (2), or never (0)
 * Unknown names and out-of-range values return GOL_ERR_INVALID.  Results are bit-identical for every setting.
 * (Test and A/B knobs -- spin limits, tag epochs, launch API -- are not board options: they live behind
 * gol_debug_set_option in the library's internal header csrc/gol_debug.h.)
 * The persistent passes (cooperative, rows-on-lanes) of all boards of a process are serialised per device, so two
 * handles stepping at once from two threads never split the CUs between two such grids.  The serialisation is per
 * PROCESS: a second process stepping a mid-size board on the same GPU at the same time can hold CUs a persistent grid
 * needs.  Its bands then wait out the spin limit (~2 s), the call's board is left wrong, and the next
 * gol_synchronize or readback returns GOL_ERR_HIP with gol_last_error() naming that cause ("a band hand-off timed
 * out -- the pass could not get every CU at once ...").  Set "coop" 0 on boards that share a GPU with other
 * processes: every generation then runs on the ordinary (non-persistent) passes. */
int gol_set_option(gol_board* b, const char* name, int64_t value);
int gol_get_option(gol_board* b, const char* name, int64_t* value);

/* ------------------------------------------------------------------------------------------------
 * A batch of small boards: `count` independent boards of one geometry, stepped by ONE launch with one wavefront per
 * board.  The reference's board is 100 x 100 and seeded from the clock (GameOfLifeLogic.fs:5,
 * GameOfLifeDriver.fs:9-11), so every run is another member of one ensemble; a batch runs thousands of members at once
 * where a gol_board handle per seed would step them one single-wave launch after another.
 *   Geometry:  the single-wave pass's -- 3 <= width <= 128 and gol_batch_supported(width, height) > 0 (the fewest rows
 *              per lane in 1..4 that divide the height with height / rows <= 64) -- anything else gol_create accepts
 *              returns GOL_ERR_UNSUPPORTED (129 x 64, 128 x 255, 100 x 257).  Both boundaries.
 *   Limits:    1 <= count <= 2^22; board ranges inside [0, count); exact buffer lengths; at most 2^26 trace entries per
 *              call -- anything else returns GOL_ERR_INVALID.  Every argument is checked before any device work.
 *   Handle:    opaque, on the calling thread's current device (no multi-GPU batches), serialised by its own mutex, with
 *              its own stream; conventions as for gol_board (codes, gol_last_error, borrowed host buffers).
 * Host buffers hold boards back to back, one byte per cell: cells[(i - first)*width*height + x + y*width].
 * A new batch is all dead.  The setters (set_cells of any range, the seeds, clear) reset the generation counter. */
typedef struct gol_batch gol_batch; /* opaque; library-owned */
/* Host-only: rows per lane (1..4) of a width x height board in a batch, or 0 when a batch does not take it. */
int gol_batch_supported(int64_t width, int64_t height);
int gol_batch_create(int64_t width, int64_t height, int boundary, int64_t count, gol_batch** out);
int gol_batch_destroy(gol_batch* b);
int gol_batch_info(gol_batch* b, int64_t* width, int64_t* height, int* boundary, int64_t* count);
/* Boards [first, first + n), n >= 1; len == n*width*height.  get_cells writes 0 / 1. */
int gol_batch_set_cells(gol_batch* b, int64_t first, int64_t n, const uint8_t* cells, int64_t len);
int gol_batch_get_cells(gol_batch* b, int64_t first, int64_t n, uint8_t* cells, int64_t len);
/* n == count; board i gets the cells gol_seed_dotnet(seeds[i], mode) gives a single board of this size. */
int gol_batch_seed_dotnet(gol_batch* b, const int32_t* seeds, int64_t n, int mode);
/* Board i gets the cells gol_seed_splitmix(seed + i) gives a single board of this size. */
int gol_batch_seed_splitmix(gol_batch* b, uint64_t seed);
int gol_batch_clear(gol_batch* b);
/* Every board advances `generations` (>= 0; 0 is a no-op) synchronous generations under the batch's rule (B3/S23
 * unless gol_ensemble_set_rule said otherwise) in one launch: a wavefront loads its board, runs every generation in
 * registers and stores it.  Asynchronous; any readback synchronises. */
int gol_batch_step(gol_batch* b, int64_t generations);
/* As gol_batch_step between two HIP timing events on the batch's stream, synchronised: the call's device time. */
int gol_batch_step_timed(gol_batch* b, int64_t generations, double* elapsed_us);
/* As gol_batch_step, sampling every board's population inside the launch: every >= 1, generations % every == 0,
 * len == (generations / every) * count <= 2^26; trace[t*count + i] = population of board i after generation
 * every*(t + 1) of this call.  A refused call leaves the boards and the generation counter untouched. */
int gol_batch_step_trace(gol_batch* b, int64_t generations, int64_t every, uint32_t* trace, int64_t len);
int gol_batch_generation(gol_batch* b, int64_t* out);
/* n == count; out[i] = population / canonical hash of board i -- the gol_population / gol_hash of a single board
 * holding the same cells. */
int gol_batch_populations(gol_batch* b, int64_t* out, int64_t n);
int gol_batch_hashes(gol_batch* b, uint64_t* out, int64_t n);
/* One board's frame, as gol_render_gray8: pixels[x + y*stride] = alive ? alive_value : 0, stride >= width. */
int gol_batch_render_gray8(gol_batch* b, int64_t board, uint8_t* pixels, int64_t stride, uint8_t alive_value);
int gol_batch_synchronize(gol_batch* b);
/* Life-like rules (B.../S...).  A rule is two 9-bit masks: bit n (0..8) of `birth` set = a dead cell with n live cells
 * among its 8 neighbours becomes alive; bit n of `survive` set = a live cell with n live neighbours stays alive.
 *   gol_rule_parse   host-only, pure.  Accepts, in any letter case and with blanks around it, "B<digits>/S<digits>",
 *     the halves swapped ("S23/B3") and the digits-only survival/birth form ("23/3"); either list may be empty
 *     ("B2/S", "B/S"); digits 0..8, each at most once per list, in any order.  Everything else -- NULL, the empty
 *     string, a 9, a repeated digit, a missing slash, a third field ("B3/S23/3"), any other character, more than 31
 *     characters -- is GOL_ERR_INVALID with both outputs untouched.
 *   gol_rule_format  host-only, pure.  The canonical "B<ascending digits>/S<ascending digits>" and its NUL; len >= 22.
 *     A mask outside 0..0x1FF or a short buffer is GOL_ERR_INVALID.  parse(format(b, s)) == (b, s) for every rule.
 *   gol_ensemble_set_rule / gol_ensemble_rule  named as gol_ensemble_cycles is: the rule is the ensemble's, and they
 *     take the batch as their argument.  Masks in 0..0x1FF, anything else GOL_ERR_INVALID with the batch's rule as it
 *     was.  A new batch is B3/S23.  The rule is a property of the handle and changes only the future: cells, the generation counter,
 *     populations and hashes are untouched, and set_cells, the seeds and clear keep it.  It is the rule of
 *     gol_batch_step, gol_batch_step_timed, gol_batch_step_trace and gol_ensemble_cycles.
 *   gol_ensemble_set_rules / gol_ensemble_rules  one rule per board: board i runs under
 *     (birth[i], survive[i]) from now on, so one batch surveys one soup under thousands of rules -- all 2^18 fit -- in
 *     one launch.  n == count, both arrays non-null, every mask in 0..0x1FF; anything else is GOL_ERR_INVALID before
 *     any device work, the whole table judged first and the batch's rules exactly as they were.  The arrays are read
 *     before the call returns; the table lives on the batch's device as count packed words, uploaded on the batch's
 *     stream before any later step.  Like the one rule it changes only the future and set_cells, the seeds and clear
 *     keep it, and it is the rule source of the same four calls; each wave reads its board's entry once, into a scalar
 *     register.  gol_ensemble_set_rule afterwards puts the batch back under one rule and the kernels it ran before.
 *     gol_ensemble_rules returns the table, or count copies of the one rule; either output may be NULL.
 *     gol_ensemble_rule on a batch with a table returns the rule all count entries agree on, or GOL_ERR_UNSUPPORTED
 *     with its outputs untouched where they differ.
 *   Boundaries: on a bounded board the cells outside are dead forever and are no cells of the board, also under a rule
 *     with B0; on a torus every cell has 8 neighbours (on a 3-wide or 3-high torus the other cells of the 3-line).
 *   gol_set_rule / gol_rule  the same for a single board (gol_board), masks as gol_rule_parse gives them.  A new board
 *     is B3/S23.  Masks outside 0..0x1FF and null outputs are GOL_ERR_INVALID with the board's rule as it was.  The
 *     rule is a property of the handle, not of the cells: gol_clear, gol_set_cells, the seeds, gol_load_packed and
 *     gol_place_rle leave it alone, and snapshots (gol_save_packed, the snapshot files) do not carry it -- whoever
 *     restores a snapshot sets the rule again.  It is the rule of gol_step and gol_step_timed; gol_pass_timing times the
 *     B3/S23 streaming pass and returns GOL_ERR_UNSUPPORTED under any other rule.  Under B3/S23 a board takes exactly
 *     the passes it always took; under another rule a board up to 128 x 256 (any height up to 256) runs the single-wave pass
 *     with the rule table, every other bit-packed board the rule-generic streaming pass (csrc/gol_rule_step.hip: 4 generations per
 *     pass over the board, any size, any layout) and the remaining byte boards one launch per generation (DESIGN.md
 *     4.12).  A board on several GPUs accepts B3/S23 only: any other rule is GOL_ERR_UNSUPPORTED, rule unchanged. */
#define GOL_RULE_LIFE_BIRTH 0x008
#define GOL_RULE_LIFE_SURVIVE 0x00C
int gol_rule_parse(const char* text, int* birth, int* survive);
int gol_rule_format(int birth, int survive, char* out, int64_t len);
int gol_ensemble_set_rule(gol_batch* b, int birth, int survive);
int gol_ensemble_rule(gol_batch* b, int* birth, int* survive);
int gol_ensemble_set_rules(gol_batch* b, const int* birth, const int* survive, int64_t n);
int gol_ensemble_rules(gol_batch* b, int* birth, int* survive, int64_t n);
int gol_set_rule(gol_board* b, int birth, int survive);
int gol_rule(gol_board* b, int* birth, int* survive);
/* Generations rules on a batch (B.../S.../C<n>): a life-like rule plus n - 2 dying states.  A cell's
 * state is s in 0 .. nstates - 1: 0 dead, 1 alive, 2 .. nstates - 1 dying; only state-1 cells count as neighbours.
 *   s = 0 -> 1 on a birth count, else 0;  s = 1 -> 1 on a survive count, else 2 (nstates > 2) or 0 (nstates = 2);
 *   s >= 2 -> s + 1 if s + 1 < nstates, else 0.  Boundaries as for any batch: outside a bounded board is state 0 forever.
 * The family's calls are gol_generations_* (as the rule's and the census's are gol_ensemble_*): they take and make
 * the same gol_batch handle, and gol_batch_* stays the plain batch's seventeen.
 *   gol_generations_create  gol_batch_create with nstates in 2..8 (else GOL_ERR_INVALID), fixed for the handle's
 *     life; nstates 2 is gol_batch_create itself and runs its kernels.  gol_generations_nstates returns it.
 *   gol_generations_set_states / gol_generations_get_states  one byte per cell holding the state, boards back to
 *     back, ranges and len as for gol_batch_set_cells.  A byte >= nstates is GOL_ERR_INVALID before any device work,
 *     batch untouched.
 *     set_states resets the generation counter.  Both work on a 2-state batch.
 *   gol_generations_parse  host-only, pure.  Everything gol_rule_parse accepts, optionally followed by a third field
 *     "/<n>", "/C<n>" or "/G<n>" (any letter case, n one digit 2..8); no third field is nstates 2.  Anything else is
 *     GOL_ERR_INVALID with all three outputs untouched.
 *   gol_generations_format  host-only, pure.  gol_rule_format's text for nstates 2, "B.../S.../C<n>" above, and its
 *     NUL; len >= GOL_GENERATIONS_FORMAT_LEN (25) whatever nstates.  A refusal writes nothing.
 * On a batch with nstates > 2: gol_ensemble_set_rule(s) / gol_ensemble_rule(s) carry birth and survive as ever (nstates
 * is batch-wide); gol_batch_step, _step_timed and _step_trace run the transition above and the trace counts state-1
 * cells; gol_batch_set_cells, both seeds and gol_batch_clear write states 0 and 1 only (a dying cell becomes dead);
 * gol_batch_get_cells, gol_batch_populations and gol_batch_render_gray8 see state 1 only; gol_batch_hashes gives board
 * i the gol_hash of a single width x (nstates - 1) * height board whose rows [(k - 1) height, k height) are the
 * indicator of state k; gol_ensemble_cycles compares whole state boards and reports the state-1 cells of B_mu. */
#define GOL_GENERATIONS_FORMAT_LEN 25
int gol_generations_create(int64_t width, int64_t height, int boundary, int64_t count, int nstates,
                                 gol_batch** out);
int gol_generations_nstates(gol_batch* b, int* nstates);
int gol_generations_set_states(gol_batch* b, int64_t first, int64_t n, const uint8_t* states, int64_t len);
int gol_generations_get_states(gol_batch* b, int64_t first, int64_t n, uint8_t* states, int64_t len);
int gol_generations_parse(const char* text, int* birth, int* survive, int* nstates);
int gol_generations_format(int birth, int survive, int nstates, char* out, int64_t len);
/* Generations rules on a single board (gol_board): the transition above at any board size.  A new board
 * has nstates 2.  The alive cells stay what every cell call of this header reads and writes: gol_get_cells,
 * gol_get_region, gol_render_gray8, gol_view_counts / gol_render_view, gol_population, gol_save_packed, the RLE text
 * see state 1 alone; gol_set_cells, gol_load_packed, both seeds and gol_clear write states 0 and 1 only (a dying cell
 * becomes dead); gol_place_rle makes the cells it places state 1.  Snapshots carry the alive cells only.
 *   gol_set_generations_rule  masks as for gol_set_rule, nstates in 2..8; anything else is GOL_ERR_INVALID and nothing
 *     changes.  The same nstates as the board has: only birth and survive change, dying cells stay.  Another nstates:
 *     every dying cell becomes dead, the alive cells and the generation counter are untouched (nstates 2: the board is
 *     a life-like board again and takes the passes it took).  GOL_ERR_OOM leaves the board as it was, nstates and rule
 *     included.  A board on several GPUs takes B3/S23 at nstates 2 only (GOL_ERR_UNSUPPORTED, board unchanged).
 *     gol_set_rule on a Generations board changes birth and survive and keeps nstates and the dying cells.
 *   gol_generations_rule  all three; gol_rule still returns the two masks.  A null output is GOL_ERR_INVALID.
 *   gol_set_states / gol_get_states  one byte per cell holding the state, len == width * height.  A byte >= nstates is
 *     GOL_ERR_INVALID before any device work, board untouched.  set_states resets the generation counter, like every
 *     setter.  Both work on a 2-state board, with states 0 and 1.
 *   On a board with nstates > 2: gol_hash is the gol_hash of a single width x (nstates - 1) * height board whose rows
 *     [(k - 1) height, k height) are the indicator of state k (what gol_batch_hashes gives a Generations batch);
 *     gol_pass_timing returns GOL_ERR_UNSUPPORTED.  Every bit-packed board runs the multi-plane streaming pass
 *     (csrc/gol_gen_stream.hip: up to 4 generations per pass over the board, any size, any layout), every byte board
 *     one launch per generation. */
int gol_set_generations_rule(gol_board* b, int birth, int survive, int nstates);
int gol_generations_rule(gol_board* b, int* birth, int* survive, int* nstates);
int gol_set_states(gol_board* b, const uint8_t* states, int64_t len);
int gol_get_states(gol_board* b, uint8_t* states, int64_t len);
/* The ensemble's cycle census: for every board, after how many generations it enters a cycle and of
 * what period, one launch, one wavefront per board, the search in that wave's registers.
 *   Definition: B_0 = board i's current cells, B_(t+1) = the next generation of B_t under the batch's rule and boundary;
 *     t* = the smallest t >= 1 with B_t = B_s for some s < t; transient mu = s, period lambda = t* - mu (minimal).
 *     Resolved, exactly when t* = mu + lambda <= max_generations: transient[i] = mu, period[i] = lambda, population[i] =
 *     live cells of B_mu.  Unresolved, exactly when t* > max_generations: transient[i] = -1, period[i] = 0,
 *     population[i] = 0.  The answer is a property of the board and max_generations, not of the search.  Cells are
 *     compared in place: a glider on a torus has the period of its return, not 4.
 *   Arguments: n == count; 1 <= max_generations <= 2^20; transient, period and population hold n entries; steps may be
 *     NULL.  Anything else returns GOL_ERR_INVALID before any device work and leaves the arrays untouched.
 *   steps[i] = generation steps the wave ran for board i: cost accounting, not a property of the board, and free to
 *     change between versions; never more than 6 * max_generations.  That is the worst case, an unresolved board, and
 *     what the cap of 2^20 bounds: a launch ends when its slowest board does (DESIGN.md 4.9 has the time of a step).
 * Read-only: the boards, the generation counter and the hashes are unchanged.  Synchronous (the results are host
 * arrays).  Not named gol_batch_*: it answers a question about the ensemble, and takes the batch as its argument. */
int gol_ensemble_cycles(gol_batch* b, int64_t max_generations, int64_t* transient, int64_t* period,
                        int64_t* population, int64_t* steps, int64_t n);

const char* gol_last_error(void);
const char* gol_version(void);
/* 1 if a device reporting this hipDeviceProp_t::gcnArchName ("gfx950", "gfx950:sramecc+:xnack-") runs this
 * build, else 0.  gol_create returns GOL_ERR_NO_DEVICE for a board on any other device. */
int gol_arch_supported(const char* gcn_arch_name);

/* ------------------------------------------------------------------------------------------------
 * Row-strip entry points for multi-GPU runs (one process per GPU; the caller owns device memory and
 * does the halo exchange, e.g. RCCL send/recv).  A strip buffer holds `ghost` halo rows, then `rows`
 * owned rows (global rows [y0, y0+rows)), then `ghost` halo rows; each buffer row is `pitch` 32-bit
 * words, of which the first width/32 are the board row in the interleaved layout `ilv`:
 *     row = blocks of ilv words; in block k, word j bit b = cell x = 32*ilv*k + j + ilv*b
 * (ilv = 1: bit b of word w = cell 32w + b).  width must be a multiple of 32*ilv, pitch of ilv.  With world size 1 a strip may instead set wrap_rows = 1, ghost = 0,
 * rows = height: torus rows then wrap inside the buffer (the single-GPU board layout).
 * `stream` is a hipStream_t (NULL = default stream).  All calls are asynchronous. */
typedef struct gol_strip {
    int64_t width;    /* global board width (cells) */
    int64_t height;   /* global board height (rows) */
    int64_t y0;       /* global row of owned row 0 */
    int64_t rows;     /* owned rows */
    int64_t ghost;    /* halo rows above and below (>= k for a k-generation pass unless wrap_rows) */
    int64_t pitch;    /* words per buffer row (>= width/32) */
    int32_t boundary; /* GOL_TORUS | GOL_BOUNDED */
    int32_t wrap_rows;
    int32_t ilv;      /* words per interleaved block: 1, 2 or 4 (gol_default_ilv) */
    int32_t spare_waves; /* waves gol_strip_step leaves free for concurrent work on other streams (e.g. the
                            halo bands of the same pass); 0 = fill the device */
} gol_strip;

/* k generations over owned rows [out_begin, out_end) from src to dst (distinct buffers, same geometry).
 * Reads rows [out_begin-k, out_end+k); with wrap_rows = 0 those must lie in [-ghost, rows+ghost), except that rows
 * beyond a bounded board's edge are dead whatever the buffer holds there (they need not exist: a bounded board in one
 * strip has ghost = 0).  The result depends on the first width/32 words of those rows only, and only the first
 * width/32 words of dst's rows [out_begin, out_end) are written: pad words (pitch > width/32, any multiple of ilv),
 * every other row of dst and all of src are left as they are.  src and dst must be aligned to 4 * ilv bytes (a lane
 * moves its block of ilv words as one load, store or LDS-DMA; any device allocation is aligned to 256) -- anything
 * else returns GOL_ERR_INVALID.  The other gol_strip_* calls move single words and take any word-aligned buffer;
 * they, too, read and write the first width/32 words of the owned rows only. */
int gol_strip_step(const gol_strip* s, const uint32_t* src, uint32_t* dst, int k, int64_t out_begin,
                   int64_t out_end, void* stream);
int gol_strip_seed_splitmix(const gol_strip* s, uint32_t* buf, uint64_t seed, void* stream);
/* cells: host or device bytes of the owned rows, cells[x + r*width] (r = owned row) */
int gol_strip_pack(const gol_strip* s, const uint8_t* dev_cells, uint32_t* buf, void* stream);
int gol_strip_unpack(const gol_strip* s, const uint32_t* buf, uint8_t* dev_cells, int64_t stride, uint8_t value,
                     void* stream);
/* Add this strip's population / canonical-hash partial sum into *dev_acc (device uint64). */
int gol_strip_population(const gol_strip* s, const uint32_t* buf, uint64_t* dev_acc, void* stream);
int gol_strip_hash_partial(const gol_strip* s, const uint32_t* buf, uint64_t* dev_acc, void* stream);
/* Row-strip primitive of gol_view_counts: ADDS the counts of this strip's OWNED rows (global rows [y0, y0+rows), never
 * its ghost rows) into dev_counts[out_w*out_h] (device uint32; the caller zeroes it, and adds the strips' buffers when
 * they live on different devices).  The view is in global board coordinates, with the rules of gol_view_counts for the
 * strip's boundary.  Asynchronous on `stream`.  Arguments are validated before the device is touched. */
int gol_strip_view_counts(const gol_strip* s, const uint32_t* buf, const gol_view* v, uint32_t* dev_counts,
                          void* stream);
/* Combine the (wrapping) sum of every strip's partial into the canonical board hash. */
uint64_t gol_hash_finalize(uint64_t partial_sum, int64_t width, int64_t height);
/* The halo messages of one pass of a multi-part board (one process, gol_create num_gpus > 1), in the order each
 * part issues them -- the plan both transports execute: op 0 = send, 1 = recv; rows are buffer rows of the part
 * (0 = the first of `ghost` halo rows).  Host-only (no device needed): tests check that every receive gets the
 * rows the topology gives it under RCCL's in-order pairing. */
typedef struct gol_xfer {
    int32_t part, op, peer, pad;
    int64_t row, nrows;
} gol_xfer;
int gol_exchange_plan(int64_t height, int boundary, int nparts, int64_t ghost, int k, gol_xfer* ops, int64_t max_ops,
                      int64_t* n_ops);
/* Number of wavefront column strips / rows per segment the step kernel uses (for roofline accounting). */
int gol_strip_plan(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t* waves,
                   int64_t* seg_rows);
/* The whole plan (n >= 8): plan[0..7] = column strips, row segments, rows per segment, seam geometry (1 / 0),
 * remainder blocks per row, remainder sub-strips per wave, packed remainder segments (segments 1 .. plan[6] share
 * remainder waves), remainder units; with n >= 10 also plan[8..9] = the SIMD groups' split and second split (1/65536
 * units, 0 = unsplit / geometric).  Planned for the current device's resident waves (4096 without a device):
 * tests/test_cpu_host.py walks it to check that no wave reads outside its buffer. */
int gol_strip_plan_ex(const gol_strip* s, int k, int64_t out_begin, int64_t out_end, int64_t* plan, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* GOL_GOL_H */
