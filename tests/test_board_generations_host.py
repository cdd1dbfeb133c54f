"""CPU tests of Generations rules on the single board (include/gol/gol.h gol_set_generations_rule, gol_generations_rule,
gol_set_states, gol_get_states): the host program tests/cpp/test_gen_board.cpp under the sanitizers, the
parser and formatter as the Python layer reaches them, the text forms Board.rule is made of, and the names in every
binding.  No kernel is launched here."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")
NAMES = ("gol_set_generations_rule", "gol_generations_rule", "gol_set_states", "gol_get_states")


def test_gen_board_under_sanitizers(tmp_path):
    """Its own main, address and undefined-behaviour sanitizers: the cell conversion of the state I/O kernels for every
    state of every nstates, the depth table of the multi-plane streaming pass, and a scalar model of one level with
    its decay planes against gen_next_cell (12 rows of one word, every nstates 3..8, 40 rules each)."""
    exe = tmp_path / "test_gen_board"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_gen_board.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cell conversion: 35 states" in r.stdout  # 2 + 3 + ... + 8
    assert "depth table: 18 entries" in r.stdout  # 3 layouts x 2 boundaries x 3 plane counts
    assert "level model: 92160 cells" in r.stdout  # 6 nstates x 40 rules x 12 rows x 32 cells
    assert "gen board ok" in r.stdout


def test_the_plan_header_has_no_hip():
    src = open(os.path.join(CSRC, "gol_gen_plan.h")).read()
    assert "#include" not in src and "__device__" not in src and "__global__" not in src
    kernel = open(os.path.join(CSRC, "gol_gen_stream.hip")).read()
    assert '#include "gol_gen_plan.h"' in kernel and '#include "gol_rule_plan.h"' in kernel
    assert '#include "gol_gen_plan.h"' in open(os.path.join(CSRC, "gol_passes.cpp")).read()


@pytest.mark.parametrize("text,want,canonical", [
    ("B2/S/3", (0x004, 0x000, 3), "B2/S/C3"),
    ("B2/S345/4", (0x004, 0x038, 4), "B2/S345/C4"),
    ("b34/s12/g3", (0x018, 0x006, 3), "B34/S12/C3"),
    (" S23/B3/C8 ", (0x008, 0x00C, 8), "B3/S23/C8"),
    ("B3/S23", (0x008, 0x00C, 2), "B3/S23"),
    ("B36/S23/2", (0x048, 0x00C, 2), "B36/S23"),
])
def test_parser_and_formatter_through_the_python_layer(text, want, canonical):
    """What Board(..., rule=...) and Board.rule are made of: _lib.generations_parse and _lib.generations_format."""
    from gameoflifewithactors_amd import _lib

    assert _lib.generations_parse(text) == want
    assert _lib.generations_format(*want) == canonical
    assert _lib.generations_parse(canonical) == want


def test_refused_texts_and_masks_are_value_errors():
    from gameoflifewithactors_amd import _lib

    for bad in ("B2/S/9", "B2/S/1", "B2/S/C", "B2/S/3/4", "B9/S/3", "B2/S/C33", ""):
        with pytest.raises(ValueError):
            _lib.generations_parse(bad)
    for bad in ((0x200, 0, 3), (8, 12, 1), (8, 12, 9)):
        with pytest.raises(ValueError):
            _lib.generations_format(*bad)


def test_board_rule_is_the_generations_formatters_text():
    """Board.rule's text forms without a device: the property formats what gol_generations_rule returns, so a two-state
    board reads "B3/S23" as before and a Generations board "B.../S.../C<n>"."""
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    class Handle(g.Board):  # a Board without a device: only the rule triple
        def __init__(self, triple):
            self._triple = triple

        def _generations_rule(self):
            return self._triple

        def close(self):
            pass

    assert Handle((8, 12, 2)).rule == "B3/S23" and Handle((8, 12, 2)).nstates == 2
    assert Handle((4, 0, 3)).rule == "B2/S/C3" and Handle((4, 0, 3)).nstates == 3
    assert Handle((0x1FF, 0x1FF, 8)).rule == "B012345678/S012345678/C8"
    assert Handle(_lib.generations_parse("B2/S345/4")).rule == "B2/S345/C4"


def test_the_calls_exist_and_refuse_a_null_board():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    assert lib.gol_set_generations_rule(None, 4, 0, 3) == _lib.GOL_ERR_INVALID
    assert b"null board" in lib.gol_last_error()
    b, s, n = ctypes.c_int(77), ctypes.c_int(78), ctypes.c_int(79)
    assert lib.gol_generations_rule(None, ctypes.byref(b), ctypes.byref(s), ctypes.byref(n)) == _lib.GOL_ERR_INVALID
    assert (b.value, s.value, n.value) == (77, 78, 79)
    assert lib.gol_set_states(None, None, 0) == _lib.GOL_ERR_INVALID
    assert lib.gol_get_states(None, None, 0) == _lib.GOL_ERR_INVALID
    assert b"null board" in lib.gol_last_error()


def test_board_generations_are_named_in_every_binding():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib, build, driver

    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    assert re.search(r"(?m)^int\s+gol_set_generations_rule\s*\(gol_board\*\s*b,\s*int birth,\s*int survive,\s*int nstates\);",
                     header)
    assert re.search(r"(?m)^int\s+gol_generations_rule\s*\(gol_board\*\s*b,\s*int\*\s*birth,\s*int\*\s*survive,\s*"
                     r"int\*\s*nstates\);", header)
    assert re.search(r"(?m)^int\s+gol_set_states\s*\(gol_board\*\s*b,\s*const uint8_t\*\s*states,\s*int64_t len\);", header)
    assert re.search(r"(?m)^int\s+gol_get_states\s*\(gol_board\*\s*b,\s*uint8_t\*\s*states,\s*int64_t len\);", header)
    fsharp = open(os.path.join(ROOT, "bindings", "fsharp", "GolNative.fs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, fsharp), name
        assert re.search(r"\b%s\(" % name, doc), name
    for attr in ("set_states", "get_states"):
        assert callable(getattr(g.Board, attr)), attr
    assert isinstance(g.Board.nstates, property) and isinstance(g.Board.rule, property)
    assert "rule" in inspect.signature(driver.run).parameters and "Generations" in driver.run.__doc__
    for fn in (g.Board.save, g.Board.from_snapshot):
        assert "alive plane only" in " ".join(fn.__doc__.split()), fn.__name__
    assert os.path.join(CSRC, "gol_gen_stream.hip") in build.SOURCES
    assert os.path.join(CSRC, "gol_gen_plan.h") in build.HEADERS


def test_the_new_pass_has_value_twelve_and_the_enumerators_stay():
    text = open(os.path.join(CSRC, "gol_board.h")).read()
    m = re.search(r"enum class Pass \{([^}]*)\}", text)
    assert [n.strip() for n in m.group(1).split(",")][-1] == "RuleStream" and len(m.group(1).split(",")) == 12
    assert re.search(r"constexpr Pass kPassGenStream = static_cast<Pass>\(12\);", text)
