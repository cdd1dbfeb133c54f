"""The poison-and-canary harness (tests/strip_arena.py) proved on the CPU, before anything runs on a GPU.

The oracle-backed engine (tests/strip_oracle_engine.py) implements the strip engine interface on CPU tensors, so the
step contract check of tests/test_gpu_strip_contract.py runs against it here: it must pass, an engine that assigns
whole packed rows (what the oracle engine did until this harness flagged it) must be reported as writing pad words, and
three planted violations must each be reported in their own class.  The GPU case table is then walked on the host:
every (ilv, k) is a depth the library runs, and the table reaches every feature of the streaming pass's plan and of
the level-pipelined pass's -- a table that never makes a remainder sub-strip fails here instead of passing quietly on
the GPU.
"""
import numpy as np
import pytest

import strip_arena as sa
from strip_oracle_engine import OracleEngine

# small strips of every kind, layout and pitch; out rows of every shape
SMALL = [
    sa.Case("wrap", 1, 4, 3, 20, "min"), sa.Case("wrap", 2, 3, 2, 17, "odd", "interior"),
    sa.Case("wrap", 4, 2, 1, 12, "min", "single"), sa.Case("tmid", 1, 3, 2, 15, "odd"),
    sa.Case("tmid", 2, 4, 3, 21, "min", "middle"), sa.Case("tmid", 4, 2, 2, 14, "tight", "top"),
    sa.Case("bwhole", 1, 5, 3, 16, "odd"), sa.Case("bwhole", 4, 3, 1, 13, "min", "interior"),
    sa.Case("bfirst", 2, 3, 2, 15, "min"), sa.Case("bfirst", 1, 4, 2, 15, "odd", "top"),
    sa.Case("blast", 2, 3, 2, 15, "odd"), sa.Case("blast", 1, 4, 3, 15, "min", "bottom"),
]
PADDED = [c for c in SMALL if c.pad != "tight"]


def test_pack_follows_the_header_layout():
    """gol.h: in block k of ilv words, word j bit b = cell 32*ilv*k + j + ilv*b -- restated here bit by bit."""
    rng = np.random.default_rng(0)
    for ilv in (1, 2, 4):
        width = 32 * ilv * 3
        cells = (rng.random((4, width)) < 0.5).astype(np.uint8)
        words = sa.pack(cells, width // 32 + ilv, ilv).view(np.uint32)
        assert not words[:, width // 32:].any()
        for blk in range(3):
            for j in range(ilv):
                for b in range(32):
                    np.testing.assert_array_equal((words[:, blk * ilv + j] >> b) & 1, cells[:, 32 * ilv * blk + j + ilv * b])
        np.testing.assert_array_equal(sa.unpack(words.view(np.int32), width, ilv), cells)


def test_arena_layout():
    g = sa.Case("tmid", 2, 3, 2, 15, "odd").geom
    a = sa.Arena(g, 11, "random")
    assert a.buf.data_ptr() % 256 == 0 and a.buf.shape == (g.buffer_rows, g.pitch)
    assert a.lead >= 11 * g.pitch and a.t.numel() - a.lead - a.buf_words >= 11 * g.pitch
    assert g.pitch % g.ilv == 0 and g.pitch % 4 != 0  # "odd": rows off a 16-byte boundary
    whole = a.read()
    np.testing.assert_array_equal(whole, a.poison)
    assert np.shares_memory(a.buf.numpy(), a.t.numpy())


@pytest.mark.parametrize("poison", sa.POISONS)
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_oracle_engine_keeps_the_step_contract(oracle, case, poison):
    rep = sa.step_contract(OracleEngine(ilv=case.ilv), case, poison)
    assert rep is None, str(rep)


class WholeRows(OracleEngine):
    """The oracle engine's `step` as it was: whole packed rows assigned, pad words zeroed."""

    def step(self, geom, src, dst, k, out_begin, out_end, stream=None, spare_waves=0):
        super().step(geom, src, dst, k, out_begin, out_end, stream, spare_waves)
        g = geom.ghost
        dst.numpy()[out_begin + g:out_end + g, geom.width // 32:] = 0


class PadWriter(OracleEngine):
    def step(self, geom, src, dst, k, out_begin, out_end, stream=None, spare_waves=0):
        super().step(geom, src, dst, k, out_begin, out_end, stream, spare_waves)
        dst.numpy()[geom.ghost + out_begin, geom.width // 32] ^= 0x10


class RowWriter(OracleEngine):
    def step(self, geom, src, dst, k, out_begin, out_end, stream=None, spare_waves=0):
        super().step(geom, src, dst, k, out_begin, out_end, stream, spare_waves)
        dst.numpy()[geom.ghost + out_end, 1] ^= 0x10  # the first owned row past the range


class PoisonReader(OracleEngine):
    def step(self, geom, src, dst, k, out_begin, out_end, stream=None, spare_waves=0):
        super().step(geom, src, dst, k, out_begin, out_end, stream, spare_waves)
        dst.numpy()[geom.ghost + out_begin, 0] |= src.numpy()[geom.ghost + out_begin, geom.width // 32]  # a pad word


@pytest.mark.parametrize("poison", ["ones", "random"])
@pytest.mark.parametrize("case", PADDED, ids=lambda c: c.id)
def test_whole_row_stores_are_flagged_as_pad_writes(oracle, case, poison):
    rep = sa.step_contract(WholeRows(ilv=case.ilv), case, poison)
    assert rep is not None and set(rep.counts) == {"pad"}, str(rep)
    ob, oe = case.out_rows
    g = case.geom
    assert all(g.ghost + ob <= r < g.ghost + oe and w >= g.width // 32 for r, w in rep.first["pad"])
    if poison == "ones":  # every pad word of the written rows
        assert rep.counts["pad"] == (oe - ob) * (g.pitch - g.width // 32)


@pytest.mark.parametrize("poison", sa.POISONS)
def test_planted_violations_are_reported_in_their_class(oracle, poison):
    case = sa.Case("tmid", 2, 3, 2, 15, "odd", "interior")
    g, (ob, oe) = case.geom, case.out_rows
    rep = sa.step_contract(PadWriter(ilv=2), case, poison)
    assert rep is not None and rep.counts == {"pad": 1} and rep.first["pad"] == [(g.ghost + ob, g.width // 32)], str(rep)
    rep = sa.step_contract(RowWriter(ilv=2), case, poison)
    assert rep is not None and rep.counts == {"row-outside-range": 1}, str(rep)
    assert rep.first["row-outside-range"] == [(g.ghost + oe, 1)]
    rep = sa.step_contract(PoisonReader(ilv=2), case, poison)
    if poison == "zeros":  # today's conditions: the read goes unseen, which is why the other two poisons exist
        assert rep is None, str(rep)
    else:
        assert rep is not None and set(rep.counts) == {"result-mismatch"}, str(rep)
        assert all(r == ob and x < 64 and x % 2 == 0 for r, x in rep.first["result-mismatch"])  # word 0 of a block


def test_stray_writes_outside_the_buffer_and_into_the_source_are_classed():
    case = sa.Case("bfirst", 1, 4, 2, 15, "min")
    src, dst, want = sa.make_step_arenas(case, "random")
    g = case.geom
    OracleEngine().step(g, src.buf, dst.buf, case.k, 0, g.rows)
    dst.t[dst.lead - 3] ^= 1
    dst.t[dst.lead + dst.buf_words + 5] ^= 1
    dst.buf[1, 0] ^= 1  # a ghost row beyond the bounded edge
    src.buf[g.ghost + 2, 1] ^= 1
    rep = sa.check(src, dst, 0, g.rows, want)
    assert rep.counts == {"guard-before": 1, "guard-after": 1, "ghost": 1, "src-modified": 1}, str(rep)
    assert rep.first == {"guard-before": [(-3,)], "guard-after": [(5,)], "ghost": [(1, 0)],
                         "src-modified": [(g.ghost + 2, 1)]}


@pytest.mark.parametrize("poison", ["ones", "random"])
def test_oracle_engine_setters_write_no_pad_word(oracle, poison):
    case = sa.Case("tmid", 2, 3, 2, 15, "odd")
    g = case.geom
    own = np.zeros((g.buffer_rows, g.pitch), bool)
    own[g.ghost:g.ghost + g.rows, :g.width // 32] = True
    cells = (np.random.default_rng(5).random((g.rows, g.width)) < 0.4).astype(np.uint8)
    for call in ("set_cells", "seed_splitmix"):
        a = sa.Arena(g, 4, poison)
        eng = OracleEngine(ilv=2)
        eng.set_cells(g, a.buf, cells) if call == "set_cells" else eng.seed_splitmix(g, a.buf, 7)
        rep = sa.Report()
        sa.check_untouched(a, own, rep)
        assert not rep.counts, f"{call}: {rep}"
        if call == "set_cells":
            np.testing.assert_array_equal(eng.get_cells(g, a.buf).numpy(), cells)


# ---------------------------------------------------------------- the GPU case table, on the host
def _lib():
    from gameoflifewithactors_amd import _lib

    return _lib.load()


def test_case_table_depths_are_supported():
    lib = _lib()
    for c in sa.CASES:
        assert lib.gol_supported_k(c.k, c.ilv) == 1, c.id
        assert 41 <= c.rows <= 150, c.id


def test_case_table_holds_what_the_issue_lists():
    t = sa.CASES
    for ilv, lo, hi in ((1, 1, 32), (2, 1, 16), (4, 1, 8)):  # each layout's shallowest and deepest streaming depth
        for k in (lo, hi):
            kinds = {c.kind for c in t if (c.ilv, c.k) == (ilv, k)}
            assert kinds == {"wrap", "tmid", "bwhole", "bfirst", "blast"}, (ilv, k, kinds)
            assert {c.pad for c in t if (c.ilv, c.k) == (ilv, k)} >= {"tight", "min"} | ({"odd"} if ilv < 4 else set())
    for k in (16, 32):
        assert {c.nblocks for c in t if c.pipe and c.k == k and c.geom.boundary == sa.TORUS} == {62, 64, 65, 94}
        assert {c.nblocks for c in t if c.pipe and c.k == k and c.geom.boundary == sa.BOUNDED} == {64, 65, 127}
        assert {c.kind for c in t if c.pipe and c.k == k} == {"wrap", "tmid", "bwhole", "bfirst", "blast"}
    for pipe in (False, True):
        mine = [c for c in t if c.pipe == pipe]
        assert {c.out for c in mine} == {"all", "interior", "single", "top", "bottom", "middle"}
        assert any(c.spare > 0 for c in mine)
        assert {c.pad for c in mine} >= {"tight", "min"}
    stream = [c for c in t if not c.pipe and c.k > 1]
    assert {5, 63, 64, 79} <= {c.nblocks for c in stream if c.geom.boundary == sa.TORUS}
    assert {5, 64, 65} <= {c.nblocks for c in stream if c.geom.boundary == sa.BOUNDED}
    for c in t:  # legal strips: the pitch a multiple of ilv, the "odd" ones off a 16-byte boundary
        g = c.geom
        assert g.pitch % g.ilv == 0 and g.pitch >= g.width // 32 and (c.pad != "odd" or g.pitch % 4)
        ob, oe = c.out_rows
        assert 0 <= ob < oe <= g.rows and (c.out in ("all", "bottom") or oe < g.rows) and (c.out in ("all", "top") or ob)


def test_case_table_reaches_every_plan_feature():
    """gol_strip_plan_ex / gol_debug_pipe_plan (host-only, planned for 4096 resident waves without a device)."""
    lib = _lib()
    seen = {n: [] for n in ("seam", "rem", "rem_p", "rem_mid", "split", "npk", "nrem", "halo-lane torus", "narrow bounded",
                            "edge-fill bounded", "pipe remainder strip")}
    for c in sa.CASES:
        p = sa.stream_plan(lib, c)
        if c.pipe:
            assert p["violations"] == 0, (c.id, p)
            seen["npk"] += [c.id] * (p["npk"] > 0)
            seen["nrem"] += [c.id] * (p["nrem"] > 0)
            seen["pipe remainder strip"] += [c.id] * (c.nblocks == 94 and p["nstrips"] == 2 and p["rem"] == 0)
            continue
        assert p["nstrips"] >= 1 and p["nsegs"] >= 1 and p["seg"] * p["nsegs"] >= c.out_rows[1] - c.out_rows[0], (c.id, p)
        seen["seam"] += [c.id] * (p["seam"] == 1)
        seen["rem"] += [c.id] * (p["rem"] > 0)
        seen["rem_p"] += [c.id] * (p["rem"] > 0 and p["rem_p"] > 1)
        seen["rem_mid"] += [c.id] * (p["rem_mid"] > 0)
        seen["split"] += [c.id] * (p["split"] > 0)
        bounded = c.geom.boundary == sa.BOUNDED
        seen["halo-lane torus"] += [c.id] * (not bounded and c.k > 1 and p["seam"] == 0)
        seen["narrow bounded"] += [c.id] * (bounded and c.k > 1 and c.nblocks < 64)
        seen["edge-fill bounded"] += [c.id] * (bounded and c.k > 1 and c.nblocks >= 64)
    missing = [n for n, ids in seen.items() if not ids]
    assert not missing, f"the case table never reaches: {missing}"
    # a remainder packed several sub-strips per wave, on ghost-row strips as well as on the single board
    packed = [sa.CASES[i] for i, c in enumerate(sa.CASES) if c.id in seen["rem_mid"]]
    assert {c.kind for c in packed} >= {"wrap", "tmid"}
