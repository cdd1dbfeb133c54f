"""Poison-and-canary arenas for the caller-owned strip entry points (include/gol/gol.h, gol_strip_*) -- test
infrastructure only, a plain helper module.

The strip entry points are the one place where a test owns the memory around a kernel.  An `Arena` is one contiguous
int32 tensor laid out as [guard | buffer_rows x pitch | guard]: the strip buffer starts at a multiple of 256 bytes
inside it, and `guard_rows` buffer rows (at the case's pitch) lie on either side.  Every word the call's contract does
not name -- pad words past width/32, rows outside the cone of the pass, ghost rows beyond a bounded board's edge, the
guards -- holds a poison: zeros (the conditions of every other test here), ones (0xFFFFFFFF, the worst case for
births) or seeded random words.  After the call `check` compares every word with what it held before.

What this can see: a stray write anywhere in either arena, and a read of a poisoned word that reaches the result (the
result then differs between poisons).  What it cannot: an access further from the buffer than the guards.  The step
tests use guard_rows = k + 8: the deepest pass reads k rows beyond its output and the level-pipelined pass's stage 0
whole trips of 4 rows, so a stray access further away than that is out of this harness's sight.

The word classes come from the gol_strip fields and (k, out_begin, out_end) alone (the header's contract); nothing
here asks the library.  Host-side pack / unpack for ilv 1 / 2 / 4 live here too, so the step tests trust neither
gol_strip_pack nor gol_strip_unpack.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from gameoflifewithactors_amd.strips import Geometry

TORUS, BOUNDED = 0, 1
POISONS = ("zeros", "ones", "random")
CLASSES = ("pad", "ghost", "row-outside-range", "guard-before", "guard-after", "src-modified", "result-mismatch")


# ---------------------------------------------------------------- host-side pack / unpack
def _cell_of_bit(width: int, ilv: int) -> np.ndarray:
    """For every stored bit position p = 32*w + b of a row: the cell it holds (include/gol/gol.h layout:
    block k of ilv words, word j bit b = cell 32*ilv*k + j + ilv*b)."""
    p = np.arange(width)
    w, b = p // 32, p % 32
    return (w // ilv) * 32 * ilv + (w % ilv) + ilv * b


def unpack(words: np.ndarray, width: int, ilv: int = 1) -> np.ndarray:
    """(rows, >= width/32) int32 -> (rows, width) uint8 cells."""
    words = np.ascontiguousarray(words)
    bits = np.unpackbits(words.astype("<u4").view(np.uint8), axis=1, bitorder="little")[:, :width]
    out = np.empty_like(bits)
    out[:, _cell_of_bit(width, ilv)] = bits
    return out


def pack(cells: np.ndarray, pitch: int, ilv: int = 1) -> np.ndarray:
    """(rows, width) uint8 cells -> (rows, pitch) int32 words, the words past width/32 zero."""
    rows, width = cells.shape
    padded = np.zeros((rows, pitch * 32), np.uint8)
    padded[:, :width] = cells[:, _cell_of_bit(width, ilv)] != 0
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


# ---------------------------------------------------------------- word classes
def row_words(geom: Geometry) -> int:
    return geom.width // 32


def cone_rows(geom: Geometry, k: int, out_begin: int, out_end: int) -> np.ndarray:
    """Buffer rows gol_strip_step may read: the cone [out_begin - k, out_end + k), wrapped if wrap_rows, cut to the
    board's rows if bounded."""
    lo, hi = out_begin - k, out_end + k
    if geom.wrap_rows:
        return np.unique(np.arange(lo, hi) % geom.rows)
    if geom.boundary == BOUNDED:
        lo, hi = max(lo, -geom.y0), min(hi, geom.height - geom.y0)
    assert -geom.ghost <= lo and hi <= geom.rows + geom.ghost, "the case breaks the header's ghost >= k rule"
    return np.arange(lo, hi) + geom.ghost


def src_contract(geom: Geometry, k: int, out_begin: int, out_end: int) -> np.ndarray:
    """(buffer_rows, pitch) bool: the words a k-generation pass over [out_begin, out_end) may read."""
    m = np.zeros((geom.buffer_rows, geom.pitch), bool)
    m[cone_rows(geom, k, out_begin, out_end), :row_words(geom)] = True
    return m


def dst_contract(geom: Geometry, out_begin: int, out_end: int) -> np.ndarray:
    """(buffer_rows, pitch) bool: the words a call writing owned rows [out_begin, out_end) may write."""
    m = np.zeros((geom.buffer_rows, geom.pitch), bool)
    m[geom.ghost + out_begin:geom.ghost + out_end, :row_words(geom)] = True
    return m


def live_rows(geom: Geometry) -> np.ndarray:
    """Buffer rows that hold rows of the board: all of them on a torus, those inside the board when bounded (the outer
    ghost rows of a first / last strip lie beyond the edge)."""
    r = np.arange(geom.buffer_rows) - geom.ghost + geom.y0
    return np.nonzero((r >= 0) & (r < geom.height))[0] if geom.boundary == BOUNDED else np.arange(geom.buffer_rows)


# ---------------------------------------------------------------- the arena
def _poison_words(poison: str, n: int, seed: int) -> np.ndarray:
    if poison == "zeros":
        return np.zeros(n, np.int32)
    if poison == "ones":
        return np.full(n, -1, np.int32)
    if poison == "random":
        return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    raise ValueError(poison)


class Arena:
    """[guard | buffer_rows x pitch | guard] int32 on `device`, every word poisoned; `buf` is the (buffer_rows, pitch)
    view a strip call gets (its data_ptr a multiple of 256).  `fill` puts contract words in; `snapshot` records what
    the arena holds before the call and `read` what it holds now (both as host arrays of the whole tensor)."""

    ALIGN = 256

    def __init__(self, geom: Geometry, guard_rows: int, poison: str, device="cpu", seed: int = 1):
        self.geom = geom
        self.guard_words = guard_rows * geom.pitch
        self.buf_words = geom.buffer_rows * geom.pitch
        slack = self.ALIGN // 4
        self.t = torch.empty(2 * self.guard_words + self.buf_words + slack, dtype=torch.int32, device=device)
        assert self.t.data_ptr() % 4 == 0
        # the first word of the buffer: the first multiple of ALIGN at or after the leading guard
        lead = self.guard_words
        lead += (-(self.t.data_ptr() + 4 * lead) % self.ALIGN) // 4
        self.lead = lead
        self.buf = self.t[lead:lead + self.buf_words].view(geom.buffer_rows, geom.pitch)
        assert self.buf.data_ptr() % self.ALIGN == 0
        self.poison = _poison_words(poison, self.t.numel(), seed)
        self.before = self.poison.copy()
        self.t.copy_(torch.from_numpy(self.before))

    def fill(self, mask: np.ndarray, words: np.ndarray) -> None:
        """buffer words under `mask` (buffer_rows, pitch) <- `words` (same shape); everything else stays poison."""
        view = self.before[self.lead:self.lead + self.buf_words].reshape(mask.shape)
        view[mask] = words[mask]
        self.t.copy_(torch.from_numpy(self.before))

    def read(self) -> np.ndarray:
        return self.t.cpu().numpy().copy()

    def buffer_of(self, whole: np.ndarray) -> np.ndarray:
        return whole[self.lead:self.lead + self.buf_words].reshape(self.geom.buffer_rows, self.geom.pitch)


@dataclass
class Report:
    """What `check` found: a count per class and the first few (buffer row, word) coordinates of each (guards: the
    word's offset from the buffer's first / past its last word; result-mismatch: (owned row, cell x))."""
    counts: dict = field(default_factory=dict)
    first: dict = field(default_factory=dict)

    def add(self, name: str, coords: np.ndarray) -> None:
        if len(coords):
            self.counts[name] = len(coords)
            self.first[name] = [tuple(int(v) for v in c) for c in coords[:6]]

    def __str__(self) -> str:
        return "; ".join(f"{n}: {c} at {self.first[n]}" for n, c in self.counts.items())


def check_untouched(arena: Arena, may_write: np.ndarray | None, rep: Report, as_src: bool = False) -> None:
    """Every word of `arena` outside `may_write` (buffer_rows, pitch; None: nothing) still holds what it held."""
    geom = arena.geom
    now, was = arena.read(), arena.before
    changed = now != was
    if as_src:
        idx = np.nonzero(changed)[0]
        off = idx - arena.lead
        rep.add("src-modified", np.stack([off // geom.pitch, off % geom.pitch], axis=1))
        return
    end = arena.lead + arena.buf_words
    rep.add("guard-before", (np.nonzero(changed[:arena.lead])[0] - arena.lead)[:, None])
    rep.add("guard-after", np.nonzero(changed[end:])[0][:, None])
    stray = arena.buffer_of(changed).copy()
    if may_write is not None:
        stray &= ~may_write
    r, w = np.nonzero(stray)
    owned = (r >= geom.ghost) & (r < geom.ghost + geom.rows)
    pad = w >= row_words(geom)
    for name, sel in (("pad", pad), ("ghost", ~pad & ~owned), ("row-outside-range", ~pad & owned)):
        rep.add(name, np.stack([r[sel], w[sel]], axis=1))


def check(src: Arena, dst: Arena, out_begin: int, out_end: int, expected: np.ndarray) -> Report | None:
    """After one step from `src` to `dst` over owned rows [out_begin, out_end): None if dst_contract, unpacked on the
    host, equals `expected` (those rows' cells), every other word of `dst` still holds its poison and `src` is
    unchanged; else a Report saying which class of word went wrong and where."""
    geom = dst.geom
    rep = Report()
    may = dst_contract(geom, out_begin, out_end)
    check_untouched(dst, may, rep)
    check_untouched(src, None, rep, as_src=True)
    got = unpack(dst.buffer_of(dst.read())[geom.ghost + out_begin:geom.ghost + out_end, :row_words(geom)],
                 geom.width, geom.ilv)
    r, x = np.nonzero(got != expected)
    rep.add("result-mismatch", np.stack([r + out_begin, x], axis=1))
    return rep if rep.counts else None


# ---------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    """One gol_strip_step call.  kind: "wrap" (torus, wrap_rows = 1), "tmid" (torus ghost-row strip, a middle strip),
    "bwhole" (bounded, the whole board in one strip, ghost 0: row -1 and row `rows` are the guards), "bfirst" /
    "blast" (bounded first / last strip with ghost = k: the outer ghost rows lie beyond the board).  pad: "tight",
    "min" (pitch = words + ilv) or "odd" (the next legal pitch that leaves rows off a 16-byte boundary; ilv 4 has
    none).  out: "all", "interior" ([a, b), a > 0, b < rows), "single" (one row), "top" / "bottom" (a band of k rows at
    an end: the multi-GPU edge launches), "middle" ([k, rows - k): their interior launch)."""
    kind: str
    ilv: int
    k: int
    nblocks: int
    rows: int
    pad: str = "tight"
    out: str = "all"
    spare: int = 0

    @property
    def id(self) -> str:
        s = f"{self.kind}-ilv{self.ilv}-k{self.k}-{self.nblocks}blk-{self.rows}rows-{self.pad}-{self.out}"
        return s + (f"-spare{self.spare}" if self.spare else "")

    @property
    def pipe(self) -> bool:
        return self.ilv == 4 and self.k in (16, 32)

    @property
    def geom(self) -> Geometry:
        words = self.nblocks * self.ilv
        pitch = words
        if self.pad == "min":
            pitch = words + self.ilv
        elif self.pad == "odd":
            assert self.ilv < 4, "a pitch that is a multiple of 4 words keeps rows on 16-byte boundaries"
            pitch = words + 2 * self.ilv
            while pitch % 4 == 0:
                pitch += self.ilv
        k, rows = self.k, self.rows
        width = 32 * words
        if self.kind == "wrap":
            return Geometry(width, rows, 0, rows, 0, pitch, TORUS, True, self.ilv)
        if self.kind == "tmid":
            return Geometry(width, rows + 2 * k + 7, k + 3, rows, k, pitch, TORUS, False, self.ilv)
        if self.kind == "bwhole":
            return Geometry(width, rows, 0, rows, 0, pitch, BOUNDED, False, self.ilv)
        if self.kind == "bfirst":
            return Geometry(width, rows + k + 5, 0, rows, k, pitch, BOUNDED, False, self.ilv)
        if self.kind == "blast":
            return Geometry(width, rows + k + 5, k + 5, rows, k, pitch, BOUNDED, False, self.ilv)
        raise ValueError(self.kind)

    @property
    def out_rows(self) -> tuple[int, int]:
        k, rows = self.k, self.rows
        return {"all": (0, rows), "interior": (7, rows - 5), "single": (rows // 2, rows // 2 + 1), "top": (0, k),
                "bottom": (rows - k, rows), "middle": (k, rows - k)}[self.out]


def _cases() -> list[Case]:
    c: list[Case] = []
    # each layout's shallowest and deepest streaming depth: every kind, at one strip plus one block (64 blocks: a seam
    # strip and a remainder block on a torus, where the depth has seam strips) or exactly one bounded edge-fill strip
    for ilv, k in ((1, 1), (1, 32), (2, 1), (2, 16), (4, 1), (4, 8)):
        odd = "odd" if ilv < 4 else "min"
        c += [Case("wrap", ilv, k, 64, 150), Case("wrap", ilv, k, 64, 150, "min"),
              Case("tmid", ilv, k, 64, 97, odd), Case("bwhole", ilv, k, 65, 97, "min"),
              Case("bfirst", ilv, k, 64, 97, odd), Case("blast", ilv, k, 65, 97)]
    # widths of the streaming pass: narrower than one wave strip, exactly one strip (63 seam blocks; 64 bounded), one
    # strip plus one block (above), a remainder of 16 blocks packed three sub-strips per wave
    for ilv, k in ((1, 8), (2, 16), (4, 8)):
        odd = "odd" if ilv < 4 else "min"
        c += [Case("wrap", ilv, k, 5, 150, odd), Case("wrap", ilv, k, 63, 150, "min"), Case("wrap", ilv, k, 79, 150),
              Case("wrap", ilv, k, 79, 150, odd), Case("tmid", ilv, k, 79, 150, "min"),
              Case("bwhole", ilv, k, 5, 97, odd), Case("bwhole", ilv, k, 64, 97, "min")]
    # output rows: the 12-wave workgroups of (12, 2) with their three-way group split, and a shallow ilv-1 pass
    for ilv, k in ((2, 12), (1, 8)):
        c += [Case("wrap", ilv, k, 79, 150, "min", "interior"), Case("wrap", ilv, k, 64, 150, "odd", "single"),
              Case("tmid", ilv, k, 79, 150, "odd", "top"), Case("tmid", ilv, k, 79, 150, "min", "bottom"),
              Case("tmid", ilv, k, 79, 150, "min", "middle", spare=64),
              Case("bfirst", ilv, k, 65, 97, "min", "top"), Case("blast", ilv, k, 65, 97, "odd", "bottom"),
              Case("bwhole", ilv, k, 65, 97, "tight", "interior")]
    # the level-pipelined pass (ilv 4, k 16 / 32): rows of 62, 64, 65 and 94 blocks on a torus, 64, 65 and 127 bounded
    for k in (16, 32):
        c += [Case("wrap", 4, k, 62, 97), Case("wrap", 4, k, 64, 97, "min"), Case("wrap", 4, k, 65, 97),
              Case("wrap", 4, k, 94, 41, "min"), Case("wrap", 4, k, 64, 150, "min", "interior"),
              Case("tmid", 4, k, 64, 97, "min"), Case("tmid", 4, k, 62, 150, "tight", "middle", spare=64),
              Case("tmid", 4, k, 65, 97, "min", "top"), Case("tmid", 4, k, 94, 97, "min", "bottom"),
              Case("tmid", 4, k, 65, 43, "min", "single"),
              Case("bwhole", 4, k, 64, 97, "min"), Case("bwhole", 4, k, 65, 41), Case("bwhole", 4, k, 127, 97, "min"),
              Case("bwhole", 4, k, 127, 97, "tight", "interior"),
              Case("bfirst", 4, k, 64, 97, "min"), Case("blast", 4, k, 127, 97, "min"),
              Case("bfirst", 4, k, 65, 97, "tight", "top"), Case("blast", 4, k, 65, 97, "min", "bottom")]
    assert len({x.id for x in c}) == len(c)
    return c


CASES = _cases()
TIGHT_ZERO_FIRST = sorted(CASES, key=lambda x: x.pad != "tight")


# ---------------------------------------------------------------- the step contract
@functools.lru_cache(maxsize=None)
def _board_and_expected(case: Case):
    """The case's random 40 % global board and its owned output rows after k generations (the oracle), computed once
    per case and shared by the three poisons; read-only."""
    import gol_oracle as o

    g = case.geom
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id))  # the same board in every process
    board = (np.random.default_rng(seed).random((g.height, g.width)) < 0.4).astype(np.uint8)
    ob, oe = case.out_rows
    want = o.c_run(board, case.k, g.boundary)[g.y0 + ob:g.y0 + oe].copy()
    board.setflags(write=False)
    want.setflags(write=False)
    return board, want


def make_step_arenas(case: Case, poison: str, device="cpu") -> tuple[Arena, Arena, np.ndarray]:
    """Source arena (the board's rows packed on the host into src_contract, poison everywhere else), destination arena
    (all poison, of another seed) and the expected output cells."""
    g = case.geom
    ob, oe = case.out_rows
    board, want = _board_and_expected(case)
    guard = case.k + 8
    src = Arena(g, guard, poison, device, seed=11)
    dst = Arena(g, guard, poison, device, seed=12)
    # buffer row r holds global row y0 + r - ghost (modulo the height on a torus); rows beyond a bounded edge hold none
    glob = np.arange(g.buffer_rows) - g.ghost + g.y0
    rows_of = np.clip(glob, 0, g.height - 1) if g.boundary == BOUNDED else glob % g.height
    src.fill(src_contract(g, case.k, ob, oe), pack(board[rows_of], g.pitch, g.ilv))
    return src, dst, want


def step_contract(engine, case: Case, poison: str, device="cpu", stream=None) -> Report | None:
    """One `engine.step` of the case between two poisoned arenas, then `check` (assertions A-C of the contract; D is A
    holding under all three poisons)."""
    src, dst, want = make_step_arenas(case, poison, device)
    ob, oe = case.out_rows
    engine.step(case.geom, src.buf, dst.buf, case.k, ob, oe, stream, spare_waves=case.spare)
    if stream is not None and hasattr(stream, "synchronize"):
        stream.synchronize()
    return check(src, dst, ob, oe, want)


# ---------------------------------------------------------------- host-only plans of the table
def stream_plan(lib, case: Case) -> dict:
    from gameoflifewithactors_amd import _lib

    s = case.geom.strip(case.spare)
    ob, oe = case.out_rows
    if case.pipe:
        p = (ctypes.c_int64 * 15)()
        rc = lib.gol_debug_pipe_plan(ctypes.byref(s), case.k, ob, oe, 0, p, 15)
        names = "nstrips rem rq rp ngroups grows pk_lo pk_hi npk nrem P split1 split2 grid violations"
    else:
        p = (ctypes.c_int64 * 10)()
        rc = lib.gol_strip_plan_ex(ctypes.byref(s), case.k, ob, oe, p, 10)
        names = "nstrips nsegs seg seam rem rem_p rem_mid rem_units split split2"
    assert rc == _lib.GOL_OK, (case.id, lib.gol_last_error())
    return dict(zip(names.split(), p))
