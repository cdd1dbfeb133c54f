"""CPU tests of the board view's host side (include/gol/gol.h gol_view_tone, gol_strip_view_counts): the tone map
against its formula, and the argument checks that run before any device work.  No kernel is launched here."""
import ctypes

import pytest

SCALES = (1, 2, 3, 64, 32768)
ALIVE = (1, 128, 255)


def _tone(count, scale, mode, alive):
    """The header's formula restated: ANY = count ? alive : 0; DENSITY = (2 count alive + n) / (2 n), n = scale^2."""
    n = scale * scale
    if mode == 0:
        return alive if count else 0
    return (2 * count * alive + n) // (2 * n)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_view_tone_matches_the_formula(mode, scale):
    from gameoflifewithactors_amd import _lib, board

    assert (_lib.VIEW_ANY, _lib.VIEW_DENSITY) == (0, 1)
    n = scale * scale
    # a pixel of n cells holds 0..n live ones (scale 1: n/2 - 1 is no count)
    counts = sorted({c for c in (0, 1, n // 2 - 1, n // 2, n - 1, n) if 0 <= c <= n})
    for alive in ALIVE:
        for c in counts:
            assert board.view_tone(c, scale, mode, alive) == _tone(c, scale, mode, alive), (c, scale, mode, alive)
        # the ends of the range: an empty pixel is black, a full one has the alive value
        assert board.view_tone(0, scale, mode, alive) == 0
        assert board.view_tone(n, scale, mode, alive) == alive


def test_view_tone_rejects_bad_mode_and_scale():
    from gameoflifewithactors_amd import board

    assert board.view_tone(5, 4, 2, 128) == 0
    assert board.view_tone(5, 0, 0, 128) == 0
    assert board.view_tone(5, 32769, 1, 128) == 0


def test_strip_view_counts_validation_without_gpu():
    """Every bad argument returns GOL_ERR_INVALID before the device is touched (there is none here)."""
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    W, H = 256, 64
    torus = _lib.Strip(width=W, height=H, y0=0, rows=H, ghost=0, pitch=W // 32, boundary=_lib.TORUS, wrap_rows=1, ilv=2)
    buf, counts = ctypes.c_void_p(256), ctypes.c_void_p(512)  # never dereferenced: validation comes first

    def call(strip, view, b=buf, c=counts):
        return lib.gol_strip_view_counts(ctypes.byref(strip) if strip is not None else None, b,
                                         ctypes.byref(view) if view is not None else None, c, None)

    ok = _lib.View(0, 0, 4, 64, 16)
    bad = {
        "scale 0": _lib.View(0, 0, 0, 4, 4),
        "scale 32769": _lib.View(0, 0, 32769, 1, 1),
        "out_w 0": _lib.View(0, 0, 1, 0, 4),
        "out_h 0": _lib.View(0, 0, 1, 4, 0),
        "out_w * out_h > 2^26": _lib.View(0, 0, 1, 1 << 14, (1 << 12) + 1),
        "torus: scale * out_w > W": _lib.View(0, 0, 4, 65, 16),
        "torus: scale * out_h > H": _lib.View(0, 0, 4, 64, 17),
        "torus: x = W": _lib.View(W, 0, 1, 4, 4),
        "torus: y = H": _lib.View(0, H, 1, 4, 4),
        "torus: x < 0": _lib.View(-1, 0, 1, 4, 4),
    }
    for what, v in bad.items():
        assert call(torus, v) == _lib.GOL_ERR_INVALID, what
        assert lib.gol_last_error()
    # the out_w * out_h limit holds for bounded strips too, whose origin may be anywhere in [-2^31, 2^31]
    bounded = _lib.Strip(width=W, height=H, y0=0, rows=H, ghost=0, pitch=W // 32, boundary=_lib.BOUNDED, wrap_rows=0,
                         ilv=2)
    assert call(bounded, _lib.View(0, 0, 1, 1 << 13, (1 << 13) + 1)) == _lib.GOL_ERR_INVALID
    assert call(bounded, _lib.View((1 << 31) + 1, 0, 1, 4, 4)) == _lib.GOL_ERR_INVALID
    assert call(bounded, _lib.View(0, -(1 << 31) - 1, 1, 4, 4)) == _lib.GOL_ERR_INVALID
    # null pointers
    assert call(None, ok) == _lib.GOL_ERR_INVALID
    assert call(torus, None) == _lib.GOL_ERR_INVALID
    assert call(torus, ok, b=None) == _lib.GOL_ERR_INVALID
    assert call(torus, ok, c=None) == _lib.GOL_ERR_INVALID
    # and a bad strip is refused as by the other strip calls
    ragged = _lib.Strip(width=100, height=H, y0=0, rows=H, ghost=0, pitch=4, boundary=0, wrap_rows=0, ilv=1)
    assert call(ragged, ok) == _lib.GOL_ERR_INVALID


def test_board_view_calls_reject_a_null_board():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    v = _lib.View(0, 0, 1, 4, 4)
    assert lib.gol_view_counts(None, ctypes.byref(v), None) == _lib.GOL_ERR_INVALID
    assert lib.gol_render_view(None, ctypes.byref(v), 0, 128, None, 4) == _lib.GOL_ERR_INVALID
