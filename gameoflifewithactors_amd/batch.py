"""BoardBatch: many independent small boards of one size, stepped together.

Reference seam: the reference's board is 100 x 100 and seeded from ``DateTime.Now.Ticks``
(``GameOfLifeLogic.fs:5``, ``GameOfLifeDriver.fs:9-11``), so every run of the app is another member of one ensemble.
One ``BoardBatch`` holds ``count`` such boards bit-packed in HBM and ``step(g)`` advances all of them ``g`` generations
in ONE launch, one wavefront per board (``csrc/gol_batch.hip``) -- where a ``Board`` per seed would
step them one single-wave launch after another.  ``step_trace`` samples every board's population inside that launch:
population curves, extinction times and soup censuses over thousands of seeds are one call.  ``cycles`` answers the
other question asked of an ensemble of soups -- after how many generations does each board settle, and into a cycle of
what period -- in one launch too: each wave runs the cycle search on the board in its registers
(``csrc/gol_cycles.hip``), where ``step(1)`` + ``hashes()`` per generation would be thousands of launches
and readbacks.  All of it runs under the batch's rule: B3/S23 unless ``rule=`` / ``set_rule`` names another life-like
rule ("B36/S23", "B3678/S34678", ...) -- or under one rule per board (``set_rules``):
one soup under thousands of rules is one launch as well.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import INIT_DOTNET_MOD2, TORUS, batch_supported, check

__all__ = ["BoardBatch", "batch_supported"]


def _u8p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _third(rule) -> bytes:
    """b"/<third field>" of a rule's text, b"" where it has two fields."""
    raw = rule.encode() if isinstance(rule, str) else rule
    return b"/" + raw.split(b"/", 2)[2] if raw.count(b"/") >= 2 else b""


class BoardBatch:
    """``count`` boards of width x height on the current HIP device.

    The geometry is the single-wave pass's: 3 <= width <= 128 and ``batch_supported(width, height) > 0`` (1 to 4 rows
    per lane on at most 64 lanes); anything else raises NotImplementedError.  boundary: ``TORUS`` or ``BOUNDED``.
    Cell arrays are ``(n, height, width)`` uint8, nonzero = alive.  rule: a life-like rule as ``set_rule`` takes it, or
    a Generations rule ("B2/S/3", "B2/S345/C4") whose third field is the number of states per cell.
    nstates (2..8, fixed for the batch's life): None takes it from the rule's text (2 without a third field); a value
    that contradicts the text raises ValueError.  With nstates > 2 a cell is dead (0), alive (1) or dying (2 ..
    nstates - 1): ``set_states`` / ``get_states`` carry the states, and cells, populations, traces and renders see
    state 1 only.
    """

    def __init__(self, width: int, height: int, count: int, boundary: int = TORUS, rule="B3/S23", nstates=None):
        self._lib = _lib.load()
        text_states = _lib.generations_parse(rule)[2] if isinstance(rule, (str, bytes)) else None
        if nstates is None:
            nstates = 2 if text_states is None else text_states
        elif text_states is not None and text_states != nstates and b"/" in _third(rule):
            raise ValueError(f"rule {rule!r} names {text_states} states, nstates={nstates}")
        h = ctypes.c_void_p()
        check(self._lib.gol_generations_create(width, height, boundary, count, nstates, ctypes.byref(h)),
              "gol_generations_create")
        self._h = h
        _lib.hold(self)
        self.width, self.height, self.count, self.boundary = width, height, count, boundary
        self.nstates = nstates
        try:
            self.set_rule(rule)
        except Exception:
            self.close()
            raise

    # ---------------------------------------------------------------- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            check(self._lib.gol_batch_destroy(self._h), "gol_batch_destroy")
            self._h = None
            _lib.release(self)

    def __enter__(self) -> "BoardBatch":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return self.count

    # ---------------------------------------------------------------- I/O
    def set_cells(self, cells, first: int = 0) -> "BoardBatch":
        """Replace boards [first, first + n) with an (n, height, width) array (a single (height, width) board is n = 1)."""
        a = np.ascontiguousarray(np.asarray(cells, dtype=np.uint8))
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.height, self.width):
            raise ValueError(f"cells must be (n, {self.height}, {self.width}), got {a.shape}")
        check(self._lib.gol_batch_set_cells(self._h, first, a.shape[0], _u8p(a), a.size), "gol_batch_set_cells")
        return self

    def get_cells(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """Boards [first, first + n) (to the end by default) as an (n, height, width) uint8 array of 0 / 1."""
        n = self.count - first if n is None else n
        out = np.empty((max(n, 0), self.height, self.width), dtype=np.uint8)
        check(self._lib.gol_batch_get_cells(self._h, first, n, _u8p(out), out.size), "gol_batch_get_cells")
        return out

    def set_states(self, states, first: int = 0) -> "BoardBatch":
        """Replace boards [first, first + n) with an (n, height, width) array of states 0 .. nstates - 1 (0 dead, 1
        alive, above dying).  A state at or above ``nstates`` raises ValueError and leaves the batch as it was.  Resets
        the generation counter."""
        a = np.asarray(states)
        if a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("states must lie in 0 .. nstates - 1")
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.height, self.width):
            raise ValueError(f"states must be (n, {self.height}, {self.width}), got {a.shape}")
        check(self._lib.gol_generations_set_states(self._h, first, a.shape[0], _u8p(a), a.size), "gol_generations_set_states")
        return self

    def get_states(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """Boards [first, first + n) (to the end by default) as an (n, height, width) uint8 array of states."""
        n = self.count - first if n is None else n
        out = np.empty((max(n, 0), self.height, self.width), dtype=np.uint8)
        check(self._lib.gol_generations_get_states(self._h, first, n, _u8p(out), out.size), "gol_generations_get_states")
        return out

    def render_gray8(self, board: int, alive_value: int = 128, stride: int | None = None) -> np.ndarray:
        """Gray8 frame of one board, pixels[x + y*stride] (Board.render_gray8)."""
        stride = self.width if stride is None else stride
        out = np.empty(max(stride, 0) * self.height, dtype=np.uint8)
        check(self._lib.gol_batch_render_gray8(self._h, board, _u8p(out), stride, alive_value),
              "gol_batch_render_gray8")
        return out

    # ---------------------------------------------------------------- seeding
    def seed_dotnet(self, seeds, mode: int = INIT_DOTNET_MOD2) -> "BoardBatch":
        """Board i <- System.Random(seeds[i]) as the reference uses it (Board.seed_dotnet); len(seeds) == count."""
        a = np.ascontiguousarray(np.asarray(seeds, dtype=np.int32)).reshape(-1)
        check(self._lib.gol_batch_seed_dotnet(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), a.size, mode),
              "gol_batch_seed_dotnet")
        return self

    def seed_splitmix(self, seed: int) -> "BoardBatch":
        """Board i <- the cells Board.seed_splitmix(seed + i) gives a single board of this size."""
        check(self._lib.gol_batch_seed_splitmix(self._h, seed & 0xFFFFFFFFFFFFFFFF), "gol_batch_seed_splitmix")
        return self

    def clear(self) -> "BoardBatch":
        check(self._lib.gol_batch_clear(self._h), "gol_batch_clear")
        return self

    # ---------------------------------------------------------------- rule
    def set_rule(self, rule) -> "BoardBatch":
        """The rule of every later ``step``, ``step_timed``, ``step_trace`` and ``cycles``: a string ("B36/S23",
        "S23/B36" or "23/36") or a ``(birth, survive)`` pair of 9-bit masks (bit n: n live neighbours).  Cells, the
        generation counter, populations and hashes are untouched, and ``set_cells``, the seeds and ``clear`` keep the
        rule.  On a bounded board the cells outside stay dead under any rule, B0 included."""
        birth, survive = self._masks(rule)
        check(self._lib.gol_ensemble_set_rule(self._h, int(birth), int(survive)), "gol_ensemble_set_rule")
        return self

    def _masks(self, rule) -> tuple:
        """(birth, survive) of a rule's text or pair.  A two-field text keeps the batch's ``nstates``; a third field
        must equal it (ValueError otherwise, as for any text the parser refuses)."""
        if not isinstance(rule, (str, bytes)):
            return int(rule[0]), int(rule[1])
        if not _third(rule):
            return _lib.rule_parse(rule)
        birth, survive, nstates = _lib.generations_parse(rule)
        if nstates != self.nstates:
            raise ValueError(f"rule {rule!r} names {nstates} states, the batch has {self.nstates}")
        return birth, survive

    @property
    def rule(self) -> str:
        """The batch's rule in canonical form, "B3/S23" for a new batch.  After ``set_rules`` it is the rule all boards
        agree on; where they differ it raises NotImplementedError (``rules`` has the list)."""
        b, s = ctypes.c_int(), ctypes.c_int()
        check(self._lib.gol_ensemble_rule(self._h, ctypes.byref(b), ctypes.byref(s)), "gol_ensemble_rule")
        return _lib.generations_format(b.value, s.value, self.nstates)

    def set_rules(self, rules) -> "BoardBatch":
        """One rule per board: board i runs every later ``step``, ``step_timed``, ``step_trace`` and ``cycles`` under
        ``rules[i]``.  ``rules`` is a sequence of ``count`` strings or ``(birth, survive)`` pairs as ``set_rule`` takes
        them, or an ``(count, 2)`` integer array of masks.  The table is checked as a whole before any of it is used: a
        wrong length or a mask outside 0..0x1FF raises ValueError and leaves the batch's rules as they were.  Like
        ``set_rule`` it changes only the future, and ``set_cells``, the seeds and ``clear`` keep it; a later
        ``set_rule`` puts the batch back under one rule."""
        if isinstance(rules, np.ndarray):
            a = rules
        else:
            a = np.array([self._masks(r) for r in rules], dtype=np.int64).reshape(-1, 2)
        if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"rules must be (n, 2) integer masks, got {a.dtype} {a.shape}")
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise ValueError("birth and survive masks must lie in 0..0x1FF")
        birth, survive = (np.ascontiguousarray(a[:, k], dtype=np.intc) for k in (0, 1))
        check(self._lib.gol_ensemble_set_rules(self._h, birth.ctypes.data_as(_lib.ip), survive.ctypes.data_as(_lib.ip),
                                               a.shape[0]), "gol_ensemble_set_rules")
        return self

    @property
    def rules(self) -> list:
        """Every board's rule in canonical form: the table of ``set_rules``, or ``count`` times the batch's one rule."""
        birth, survive = (np.empty(self.count, dtype=np.intc) for _ in range(2))
        check(self._lib.gol_ensemble_rules(self._h, birth.ctypes.data_as(_lib.ip), survive.ctypes.data_as(_lib.ip),
                                           self.count), "gol_ensemble_rules")
        pairs = list(zip(birth.tolist(), survive.tolist()))
        text = {k: _lib.generations_format(*k, self.nstates) for k in set(pairs)}  # a table names few distinct rules, 2^18 at the most
        return [text[k] for k in pairs]

    # ---------------------------------------------------------------- stepping
    def step(self, generations: int = 1) -> "BoardBatch":
        check(self._lib.gol_batch_step(self._h, generations), "gol_batch_step")
        return self

    def step_timed(self, generations: int) -> float:
        """gol_batch_step between HIP timing events on the batch's stream, synchronised: microseconds of device time."""
        us = ctypes.c_double()
        check(self._lib.gol_batch_step_timed(self._h, generations, ctypes.byref(us)), "gol_batch_step_timed")
        return us.value

    def step_trace(self, generations: int, every: int = 1) -> np.ndarray:
        """Advance `generations` (a multiple of `every`) and return the (generations // every, count) uint32 populations
        after every `every`-th generation of this call, sampled inside the one launch."""
        t = max(generations, 0) // every if every >= 1 else 0  # (the library refuses what does not divide)
        out = np.empty((t, self.count), dtype=np.uint32)
        check(self._lib.gol_batch_step_trace(self._h, generations, every, out.ctypes.data_as(_lib.u32p), out.size),
              "gol_batch_step_trace")
        return out

    def synchronize(self) -> None:
        check(self._lib.gol_batch_synchronize(self._h), "gol_batch_synchronize")

    @property
    def generation(self) -> int:
        v = ctypes.c_int64()
        check(self._lib.gol_batch_generation(self._h, ctypes.byref(v)), "gol_batch_generation")
        return v.value

    # ---------------------------------------------------------------- observables
    def populations(self) -> np.ndarray:
        """(count,) int64: live cells of every board."""
        out = np.empty(self.count, dtype=np.int64)
        check(self._lib.gol_batch_populations(self._h, out.ctypes.data_as(_lib.i64p), out.size),
              "gol_batch_populations")
        return out

    def hashes(self) -> np.ndarray:
        """(count,) uint64: the canonical hash of every board (Board.hash of a single board with the same cells)."""
        out = np.empty(self.count, dtype=np.uint64)
        check(self._lib.gol_batch_hashes(self._h, out.ctypes.data_as(_lib.u64p), out.size), "gol_batch_hashes")
        return out

    def cycles(self, max_generations: int, with_steps: bool = False):
        """The cycle every board's current cells run into, searched for ``max_generations`` generations at most
        (1 .. 2**20): ``(transient, period, population)``, each a (count,) int64 array, and ``steps`` as a fourth when
        ``with_steps``.

        For board i let B_0 be its current cells and B_{t+1} the next generation of B_t under the batch's rule and
        boundary, t* the smallest t >= 1 with B_t == B_s for some s < t, mu = s (the transient) and lambda = t* - mu (the
        period, minimal by construction).  Resolved, exactly when t* = mu + lambda <= max_generations:
        ``transient[i] = mu``, ``period[i] = lambda``, ``population[i]`` = live cells of B_mu.  Unresolved, exactly when
        t* > max_generations: ``(-1, 0, 0)``.  The answer depends on the board and ``max_generations`` only, never on
        how the search went.  Cells are compared in place: under B3/S23 a glider on a 100 x 100 torus is
        ``(0, 400, 5)``, a still life ``(0, 1, population)``, an empty board ``(0, 1, 0)`` (under ``B0/S`` it is
        ``(0, 2, 0)``).

        Read-only: cells, hashes and ``generation`` are unchanged.  ``steps[i]`` is the number of generation steps the
        wave ran for board i -- cost accounting, not a property of the board, free to change between versions, never
        above ``6 * max_generations`` (the worst case: an unresolved board)."""
        out = [np.empty(self.count, dtype=np.int64) for _ in range(4 if with_steps else 3)]
        ptrs = [a.ctypes.data_as(_lib.i64p) for a in out] + ([] if with_steps else [None])
        check(self._lib.gol_ensemble_cycles(self._h, max_generations, *ptrs, self.count), "gol_ensemble_cycles")
        return tuple(out)

    def info(self) -> dict:
        w, h, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        b = ctypes.c_int()
        check(self._lib.gol_batch_info(self._h, ctypes.byref(w), ctypes.byref(h), ctypes.byref(b), ctypes.byref(c)),
              "gol_batch_info")
        return {"width": w.value, "height": h.value, "boundary": b.value, "count": c.value,
                "rows_per_lane": batch_supported(w.value, h.value)}
