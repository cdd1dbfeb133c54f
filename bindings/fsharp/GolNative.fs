// GolNative.fs -- F# P/Invoke binding of libgol_hip.so (include/gol/gol.h), for the reference's
// GameOfLife / GameOfLifeAkka projects (add before GameOfLifeDriver.fs in GameOfLife.fsproj:59-65).
// Not compiled in this repository (no dotnet in the build image); the same entry points are exercised
// through ctypes by tests/. See INTEGRATION.md.
module GolNative

open System
open System.Runtime.InteropServices

[<Literal>]
let Lib = "gol_hip"   // libgol_hip.so (Linux) / gol_hip.dll; ships next to the executable

type Boundary = Torus = 0 | Bounded = 1          // GameOfLifeDriver.fs:25 | Script.fsx:11
type InitMode = DotNetMod2 = 0 | DotNetNext2 = 1 // GameOfLifeDriver.fs:9-11,16-19 | Script.fsx:25-27

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_create(int64 width, int64 height, int boundary, int numGpus, int tblockK, nativeint& board)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_destroy(nativeint board)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_set_cells(nativeint board, byte[] cells, int64 len)        // cells.[x + y*W], 0/1
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_get_cells(nativeint board, byte[] cells, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_seed_dotnet(nativeint board, int seed, int mode)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_step(nativeint board, int64 generations)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_render_gray8(nativeint board, byte[] pixels, int64 stride, byte aliveValue)
/// gol_view: pixel (i, j) covers the Scale x Scale cells from (X + Scale*i, Y + Scale*j)
[<Struct; StructLayout(LayoutKind.Sequential)>]
type GolView =
    val mutable X: int64
    val mutable Y: int64
    val mutable Scale: int64
    val mutable OutW: int64
    val mutable OutH: int64
type ViewMode = Any = 0 | Density = 1            // GOL_VIEW_ANY | GOL_VIEW_DENSITY
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_view_counts(nativeint board, GolView& view, uint32[] counts)   // counts.[i + j*OutW]
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_render_view(nativeint board, GolView& view, int mode, byte aliveValue, byte[] pixels, int64 stride)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern byte gol_view_tone(uint32 count, int64 scale, int mode, byte aliveValue)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_save_packed(nativeint board, uint64[] words, int64 len)   // canonical snapshot, H*ceil(W/64)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_load_packed(nativeint board, uint64[] words, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_population(nativeint board, int64& out)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_hash(nativeint board, uint64& out)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_synchronize(nativeint board)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_set_option(nativeint board, [<MarshalAs(UnmanagedType.LPStr)>] string name, int64 value)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_transport(nativeint board, int& transport, System.Text.StringBuilder note, int64 noteLen)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_step_timed(nativeint board, int64 generations, double& elapsedUs)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_device_count(int& n)
// ---- batches of small boards (gol.h gol_batch_*): one wavefront per board, every board stepped by one launch
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_supported(int64 width, int64 height)   // host-only: rows per lane (1..4), 0 = not a batch geometry
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_create(int64 width, int64 height, int boundary, int64 count, nativeint& batch)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_destroy(nativeint batch)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_info(nativeint batch, int64& width, int64& height, int& boundary, int64& count)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_set_cells(nativeint batch, int64 first, int64 n, byte[] cells, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_get_cells(nativeint batch, int64 first, int64 n, byte[] cells, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_seed_dotnet(nativeint batch, int[] seeds, int64 n, int mode)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_seed_splitmix(nativeint batch, uint64 seed)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_clear(nativeint batch)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_step(nativeint batch, int64 generations)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_step_timed(nativeint batch, int64 generations, double& elapsedUs)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_step_trace(nativeint batch, int64 generations, int64 every, uint32[] trace, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_generation(nativeint batch, int64& generation)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_populations(nativeint batch, int64[] populations, int64 n)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_hashes(nativeint batch, uint64[] hashes, int64 n)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_render_gray8(nativeint batch, int64 board, byte[] pixels, int64 stride, byte aliveValue)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_batch_synchronize(nativeint batch)
// the ensemble's cycle census (gol.h): transient, period and population of every board's cycle within maxGenerations;
// steps may be null
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_ensemble_cycles(nativeint batch, int64 maxGenerations, int64[] transient, int64[] period, int64[] population, int64[] steps, int64 n)
// life-like rules (gol.h): two 9-bit masks, bit n = n live neighbours; parse / format are host-only; the batch's rule
// (B3/S23 until set) is the rule of step, step_timed, step_trace and the census
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl, CharSet = CharSet.Ansi)>]
extern int gol_rule_parse(string text, int& birth, int& survive)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_rule_format(int birth, int survive, byte[] out, int64 len)   // len >= 22
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_ensemble_set_rule(nativeint batch, int birth, int survive)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_ensemble_rule(nativeint batch, int& birth, int& survive)
// ... one rule per board (n = count entries each): board i runs under (birth[i], survive[i]); gol_ensemble_rules
// returns the table, or count copies of the one rule, and either of its arrays may be null
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_ensemble_set_rules(nativeint batch, int[] birth, int[] survive, int64 n)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_ensemble_rules(nativeint batch, int[] birth, int[] survive, int64 n)
// ... Generations rules (B/S/C<n>): a batch of nstates 2..8 states per cell, its state bytes and the rule's text
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_create(int64 width, int64 height, int boundary, int64 count, int nstates, nativeint& out)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_nstates(nativeint batch, int& nstates)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_set_states(nativeint batch, int64 first, int64 n, byte[] states, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_get_states(nativeint batch, int64 first, int64 n, byte[] states, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl, CharSet = CharSet.Ansi)>]
extern int gol_generations_parse(string text, int& birth, int& survive, int& nstates)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_format(int birth, int survive, int nstates, byte[] out, int64 len)   // len >= 25
// ... and of a single board (B3/S23 until set; boards on several GPUs take B3/S23 only)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_set_rule(nativeint board, int birth, int survive)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_rule(nativeint board, int& birth, int& survive)
// ... Generations rules of a single board (nstates 2..8; one state byte per cell; boards on several GPUs stay at 2)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_set_generations_rule(nativeint board, int birth, int survive, int nstates)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_generations_rule(nativeint board, int& birth, int& survive, int& nstates)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_set_states(nativeint board, byte[] states, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gol_get_states(nativeint board, byte[] states, int64 len)
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern nativeint gol_last_error()

let check (what: string) rc =
    if rc <> 0 then
        failwithf "%s failed (%d): %s" what rc (Marshal.PtrToStringAnsi(gol_last_error()))

/// One board in HBM: replaces the W*H cell agents (GameOfLifeLogic.fs:39-71).  numGpus > 1 spreads it
/// over GPUs 0..numGpus-1 of this process as row strips (bit-identical; width must be a multiple of 32).
type Board(width: int, height: int, boundary: Boundary, ?numGpus: int) =
    let mutable h = 0n
    do check "gol_create" (gol_create(int64 width, int64 height, int boundary, defaultArg numGpus 1, 0, &h))
    member _.Seed(seed: int, mode: InitMode) = check "gol_seed_dotnet" (gol_seed_dotnet(h, seed, int mode))
    member _.Step(generations: int64) = check "gol_step" (gol_step(h, generations))
    /// "B36/S23", "S23/B36" or "23/36": the rule of every later Step (B3/S23 until set)
    member _.SetRule(rule: string) =
        let mutable birth = 0
        let mutable survive = 0
        check "gol_rule_parse" (gol_rule_parse(rule, &birth, &survive))
        check "gol_set_rule" (gol_set_rule(h, birth, survive))
    member _.GetCells() =
        let a = Array.zeroCreate<byte> (width * height)
        check "gol_get_cells" (gol_get_cells(h, a, int64 a.Length)); a
    member _.Render(pixels: byte[], alive: byte) =
        check "gol_render_gray8" (gol_render_gray8(h, pixels, int64 width, alive))
    /// Gray8 frame of a view (x, y, scale, outW, outH) into pixels.[i + j*outW]: the zoomed-out or panned picture
    /// of a board too large to show cell by cell (GameOfLifeUI.fs:21-31 at one pixel per scale x scale cells).
    member _.RenderView(x: int64, y: int64, scale: int64, outW: int, outH: int, mode: ViewMode, alive: byte,
                        pixels: byte[]) =
        let mutable v = GolView(X = x, Y = y, Scale = scale, OutW = int64 outW, OutH = int64 outH)
        check "gol_render_view" (gol_render_view(h, &v, int mode, alive, pixels, int64 outW))
    member _.ViewCounts(x: int64, y: int64, scale: int64, outW: int, outH: int) =
        let mutable v = GolView(X = x, Y = y, Scale = scale, OutW = int64 outW, OutH = int64 outH)
        let c = Array.zeroCreate<uint32> (outW * outH)
        check "gol_view_counts" (gol_view_counts(h, &v, c)); c
    member _.Save() =   // 1 bit per cell, layout- and GPU-count-independent
        let w = Array.zeroCreate<uint64> (height * ((width + 63) / 64))
        check "gol_save_packed" (gol_save_packed(h, w, int64 w.Length)); w
    member _.Load(words: uint64[]) = check "gol_load_packed" (gol_load_packed(h, words, int64 words.Length))
    /// gol_step timed by the library's own HIP events (device microseconds of the call): the host's own figure,
    /// under the HIP runtime the library links -- no other GPU runtime in the F# process.
    member _.StepTimed(generations: int64) =
        let mutable us = 0.0
        check "gol_step_timed" (gol_step_timed(h, generations, &us)); us
    /// Wait for the board's work; reports a failed cooperative pass (GOL_ERR_HIP) like every readback.
    member _.Synchronize() = check "gol_synchronize" (gol_synchronize h)
    /// Path / tuning option (gol.h lists the names, e.g. "coop" 0); results are bit-identical for every setting.
    member this.SetOption(name: string, value: int64) =
        check "gol_set_option" (gol_set_option(h, name, value)); this
    /// Halo transport of a multi-GPU board: 0 none (one part), 1 peer copies (the default), 2 RCCL (after
    /// SetOption("transport", 2L), one strip per GPU); with a description.
    member _.Transport() =
        let mutable t = 0
        let note = System.Text.StringBuilder(256)
        check "gol_transport" (gol_transport(h, &t, note, int64 note.Capacity)); (t, note.ToString())
    interface IDisposable with
        member _.Dispose() = if h <> 0n then (gol_destroy h |> ignore; h <- 0n)

/// `count` boards of the reference's size (any width 3..128 with gol_batch_supported > 0) stepped together: the ensemble
/// the reference samples one clock seed at a time (GameOfLifeDriver.fs:9-11).  Board i is seeded like Board.Seed(seeds.[i]).
type Batch(width: int, height: int, count: int, boundary: Boundary) =
    let mutable h = 0n
    do check "gol_batch_create" (gol_batch_create(int64 width, int64 height, int boundary, int64 count, &h))
    member _.Count = count
    member _.Seed(seeds: int[], mode: InitMode) =
        check "gol_batch_seed_dotnet" (gol_batch_seed_dotnet(h, seeds, int64 seeds.Length, int mode))
    /// "B36/S23", "S23/B36" or "23/36": the rule of every later Step / StepTrace (B3/S23 until set)
    member _.SetRule(rule: string) =
        let mutable birth = 0
        let mutable survive = 0
        check "gol_rule_parse" (gol_rule_parse(rule, &birth, &survive))
        check "gol_ensemble_set_rule" (gol_ensemble_set_rule(h, birth, survive))
    member _.Step(generations: int64) = check "gol_batch_step" (gol_batch_step(h, generations))
    /// Steps and returns trace.[t * count + i] = population of board i after generation every * (t + 1) of this call.
    member _.StepTrace(generations: int64, every: int64) =
        let t = Array.zeroCreate<uint32> (int (generations / every) * count)
        check "gol_batch_step_trace" (gol_batch_step_trace(h, generations, every, t, int64 t.Length)); t
    member _.Populations() =
        let p = Array.zeroCreate<int64> count
        check "gol_batch_populations" (gol_batch_populations(h, p, int64 count)); p
    member _.Hashes() =
        let p = Array.zeroCreate<uint64> count
        check "gol_batch_hashes" (gol_batch_hashes(h, p, int64 count)); p
    /// One board's Gray8 frame for the render agent (GameOfLifeUI.fs:24-28).
    member _.Render(board: int, pixels: byte[], alive: byte) =
        check "gol_batch_render_gray8" (gol_batch_render_gray8(h, int64 board, pixels, int64 width, alive))
    member _.GetCells(first: int, n: int) =
        let a = Array.zeroCreate<byte> (n * width * height)
        check "gol_batch_get_cells" (gol_batch_get_cells(h, int64 first, int64 n, a, int64 a.Length)); a
    interface IDisposable with
        member _.Dispose() = if h <> 0n then (gol_batch_destroy h |> ignore; h <- 0n)

/// A new Gray8 frame (outW * outH bytes) of the view: what the render agent writes to its bitmap per tick.
let renderView (board: Board) (x: int64, y: int64, scale: int64, outW: int, outH: int) (mode: ViewMode) (alive: byte) =
    let pixels = Array.zeroCreate<byte> (outW * outH)
    board.RenderView(x, y, scale, outW, outH, mode, alive, pixels)
    pixels
