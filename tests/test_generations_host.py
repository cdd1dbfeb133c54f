"""CPU tests of Generations rules (B/S/C): the bit-sliced transition, the three-field parser and the
formatter under the sanitizers (tests/cpp/test_generations.cpp), the same parser through ctypes, and the numpy reference
of tests/test_gpu_generations.py against tests/rule_reference.py at 2 states.  No kernel is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import generations_reference as gref
import rule_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("gol_generations_create", "gol_generations_nstates", "gol_generations_set_states", "gol_generations_get_states",
         "gol_generations_parse", "gol_generations_format")


def test_generations_under_sanitizers(tmp_path):
    """Its own main, address and undefined-behaviour sanitizers: rule_next_row + gen_decay equal the scalar definition
    for every nstates, state, neighbour count and value of the deciding rule bit with the word's 32 cells in mixed
    states, and on 4000 random rules; format then parse is the identity; refused texts leave the outputs untouched."""
    exe = tmp_path / "test_generations"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_generations.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "generations transition: 6520 words" in r.stdout  # (2+..+8) states x 9 x 2 x 4 + 4000
    assert "generations ok" in r.stdout


def test_parse_and_format_through_ctypes():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    assert _lib.generations_parse("B2/S/3") == (4, 0, 3) == _lib.generations_parse(" b2/s/c3 ")
    assert _lib.generations_parse("B2/S345/G4") == (4, 0x38, 4) and _lib.generations_parse("S23/B3/8") == (8, 12, 8)
    assert _lib.generations_parse("B36/S23") == (0x48, 12, 2) == _lib.generations_parse(b"B36/S23/2")
    assert _lib.generations_format(4, 0, 3) == "B2/S/C3" and _lib.generations_format(8, 12, 2) == "B3/S23"
    assert _lib.generations_format(0x1FF, 0x1FF, 8) == "B012345678/S012345678/C8"
    rng = np.random.default_rng(5)
    for birth, survive, n in zip(rng.integers(0, 512, 300), rng.integers(0, 512, 300), rng.integers(2, 9, 300)):
        text = _lib.generations_format(int(birth), int(survive), int(n))
        assert _lib.generations_parse(text) == (birth, survive, n)
        assert (text == _lib.rule_format(int(birth), int(survive))) == (n == 2)
    for text in ("", "B3/S23/", "B3/S23/1", "B3/S23/9", "B3/S23/C", "B3/S23/3/4", "B3/S23/x3", "B3/S23/33", "B9/S2/3",
                 "B3/S23/3" + " " * 24):
        out = [ctypes.c_int(-5), ctypes.c_int(-6), ctypes.c_int(-7)]
        assert lib.gol_generations_parse(text.encode(), *map(ctypes.byref, out)) == _lib.GOL_ERR_INVALID, text
        assert lib.gol_last_error().startswith(b"rule: ") and [o.value for o in out] == [-5, -6, -7], text
        with pytest.raises(ValueError, match="rule"):
            _lib.generations_parse(text)
    buf = ctypes.create_string_buffer(b"?" * 40, 41)
    for args in ((8, 12, 3, buf, 24), (8, 12, 1, buf, 40), (8, 12, 9, buf, 40), (512, 0, 3, buf, 40), (8, 12, 3, None, 40)):
        assert lib.gol_generations_format(*args) == _lib.GOL_ERR_INVALID, args[:3]
        assert buf.raw[:40] == b"?" * 40
    assert lib.gol_generations_format(0x1FF, 0x1FF, 8, buf, 25) == 0
    assert buf.raw[:26] == b"B012345678/S012345678/C8\0?"  # 25 bytes written, not one more
    with pytest.raises(ValueError, match="rule"):  # the two-field parser is as it was
        _lib.rule_parse("B3/S23/3")


def test_generations_are_named_in_every_binding():
    from gameoflifewithactors_amd import _lib, build

    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "gol", "gol.h")).read()
    fsharp = open(os.path.join(root, "bindings", "fsharp", "GolNative.fs")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in header, name
        assert "extern int %s(" % name in fsharp, name
    assert "#define GOL_GENERATIONS_FORMAT_LEN 25" in header
    csrc = os.path.join(root, "gameoflifewithactors_amd", "csrc")
    for name in ("gol_generations.h", "gol_batch_wave.h"):
        assert os.path.join(csrc, name) in build.HEADERS, name
    assert '#include "gol_generations.h"' in open(os.path.join(csrc, "gol_batch_wave.h")).read()
    for name in ("gol_batch.hip", "gol_cycles.hip"):  # the step and the census kernels of the family
        assert os.path.join(csrc, name) in build.SOURCES
        assert '#include "gol_batch_wave.h"' in open(os.path.join(csrc, name)).read(), name
    assert lib.gol_generations_nstates(None, None) == _lib.GOL_ERR_INVALID
    assert lib.gol_generations_set_states(None, 0, 1, None, 0) == _lib.GOL_ERR_INVALID


@pytest.mark.parametrize("boundary", [0, 1])
@pytest.mark.parametrize("rule", ["B3/S23", "B36/S23", "B2/S"])
def test_the_reference_at_two_states_is_the_life_like_reference(rule, boundary):
    birth, survive, n = gref.masks(rule)
    assert n == 2 and (birth, survive) == ref.masks(rule)
    for w, h, seed in ((3, 3, 1), (33, 12, 2), (100, 100, 3)):
        cells = ref.soup(w, h, seed)
        for g in (1, 7):
            assert np.array_equal(gref.gen_step(cells, birth, survive, 2, boundary, g),
                                  ref.ref_step(cells, birth, survive, boundary, g)), (w, h, g)


def test_all_alive_bounded_board_blinks_through_its_dying_states():
    s = np.ones((5, 7), dtype=np.uint8)
    birth, survive, n = gref.masks("B012345678/S/4")
    counts = []
    for _ in range(7):
        counts.append(int((s == 1).sum()))
        s = gref.gen_step(s, birth, survive, n, 1, 1)
    assert counts == [35, 0, 0, 0, 35, 0, 0]
    assert gref.gen_cycles(np.ones((5, 7), dtype=np.uint8), birth, survive, n, 1, 10) == (0, 4, 35)
    assert gref.stacked(np.array([[0, 1, 2, 3]]), 4).tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
