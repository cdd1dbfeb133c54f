"""What the caller-owned strip entry points (include/gol/gol.h, gol_strip_*) touch, word by word.

Every other parity test runs in the same memory conditions: zeroed buffers, pitch == width / 32, and nobody looks at
memory a call was not supposed to touch.  Here each call runs between poisoned arenas (tests/strip_arena.py): pad
words, rows outside the pass's cone, ghost rows beyond a bounded board's edge and guard rows around the buffer hold
zeros, ones or random words, the board is packed and unpacked on the host, and after the call

    A. the words the call may write, unpacked on the host, equal the oracle;
    B. every other word of the destination arena is bit-identical to its poison;
    C. the whole source arena is unchanged;
    D. (A under all three poisons) nothing the call may not read reaches the result.

The step cases are the smallest shapes at which each geometry of the streaming pass (csrc/gol_step.hip) and of the
level-pipelined pass (csrc/gol_pipe.hip) exists; tests/test_strip_arena.py checks on the host that the table reaches
every plan feature.  The tight-pitch, zero-poison cases -- the conditions of the other tests -- run first.
"""
import ctypes

import numpy as np
import pytest
import torch

import strip_arena as sa

pytestmark = pytest.mark.gpu

A5 = 0xA5


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


@pytest.fixture(scope="module")
def hip(gol):
    """(engine, stream, device, lib): the product's strip engine on the stream the arenas are filled on."""
    from gameoflifewithactors_amd import _lib
    from gameoflifewithactors_amd.strips import HipEngine

    dev = torch.device("cuda", torch.cuda.current_device())
    with HipEngine(dev) as eng:
        yield eng, torch.cuda.current_stream(dev), dev, _lib.load()


def _pipe_errors(lib):
    v = ctypes.c_int()
    assert lib.gol_debug_pipe_errors(ctypes.byref(v)) == 0
    return v.value


# the conditions that pass today first, then the rest
STEP = [(c, "zeros") for c in sa.CASES if c.pad == "tight"]
STEP += [(c, p) for c in sa.CASES for p in sa.POISONS if (c, p) not in STEP]


@pytest.mark.parametrize("case,poison", STEP, ids=lambda v: v.id if isinstance(v, sa.Case) else v)
def test_strip_step_contract(hip, oracle, case, poison):
    eng, stream, dev, lib = hip
    rep = sa.step_contract(eng, case, poison, dev, stream)
    assert rep is None, f"{case.id} {poison}: {rep}"
    if case.pipe:
        assert _pipe_errors(lib) == 0


# ---------------------------------------------------------------- the other strip entry points
K = 3  # ghost rows of the strips below (no pass runs on them)


def _board_strips(ilv, boundary, pad, nblocks=5, rows=(14, 13, 15)):
    """A board cut into three ghost-row strips (first, middle, last), pitch tight or padded."""
    words = nblocks * ilv
    pitch = {"tight": words, "min": words + ilv, "odd": words + 3 * ilv}[pad]
    height = sum(rows)
    y0 = np.concatenate([[0], np.cumsum(rows)])
    return [sa.Geometry(32 * words, height, int(y0[i]), rows[i], K, pitch, boundary, False, ilv) for i in range(3)]


def _owned(g):
    m = np.zeros((g.buffer_rows, g.pitch), bool)
    m[g.ghost:g.ghost + g.rows, :g.width // 32] = True
    return m


def _filled(g, cells_owned, poison, dev, seed=21):
    """An arena holding the strip's owned rows (packed on the host); pad words, ghost rows and guards poisoned."""
    a = sa.Arena(g, 4, poison, dev, seed=seed)
    full = np.zeros((g.buffer_rows, g.pitch), np.int32)
    full[g.ghost:g.ghost + g.rows] = sa.pack(cells_owned, g.pitch, g.ilv)
    a.fill(_owned(g), full)
    return a


def _assert_untouched(arena, may_write, what):
    rep = sa.Report()
    sa.check_untouched(arena, may_write, rep)
    assert not rep.counts, f"{what}: {rep}"


LAYOUTS = [(1, "tight"), (1, "min"), (1, "odd"), (2, "tight"), (2, "min"), (2, "odd"), (4, "tight"), (4, "min")]


def _board(g, seed):
    return (np.random.default_rng(seed).random((g.height, g.width)) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("poison", sa.POISONS)
@pytest.mark.parametrize("ilv,pad", LAYOUTS)
def test_strip_pack_and_seed_write_the_owned_words_only(hip, oracle, ilv, pad, poison):
    eng, stream, dev, lib = hip
    for boundary in (sa.TORUS, sa.BOUNDED):
        geoms = _board_strips(ilv, boundary, pad)
        board = _board(geoms[0], 7 + ilv)
        seeded = oracle.seed_splitmix(geoms[0].width, geoms[0].height, 99)
        for g in geoms:
            words = g.width // 32
            for what, cells in (("pack", board), ("seed", seeded)):
                a = sa.Arena(g, 4, poison, dev, seed=31)
                s = g.strip()
                if what == "pack":
                    src = torch.from_numpy(np.ascontiguousarray(cells[g.y0:g.y0 + g.rows])).to(dev)
                    rc = lib.gol_strip_pack(ctypes.byref(s), src.data_ptr(), a.buf.data_ptr(), stream.cuda_stream)
                else:
                    rc = lib.gol_strip_seed_splitmix(ctypes.byref(s), a.buf.data_ptr(), 99, stream.cuda_stream)
                assert rc == 0, lib.gol_last_error()
                stream.synchronize()
                _assert_untouched(a, _owned(g), f"{what} y0={g.y0} boundary={boundary}")
                got = a.buffer_of(a.read())[g.ghost:g.ghost + g.rows, :words]
                np.testing.assert_array_equal(got, sa.pack(cells[g.y0:g.y0 + g.rows], words, ilv), err_msg=what)


@pytest.mark.parametrize("value", [1, 255])
@pytest.mark.parametrize("poison", sa.POISONS)
@pytest.mark.parametrize("ilv,pad", LAYOUTS)
def test_strip_unpack_reads_the_owned_words_and_writes_the_cells_only(hip, ilv, pad, poison, value):
    eng, stream, dev, lib = hip
    g = _board_strips(ilv, sa.BOUNDED, pad)[1]
    cells = _board(g, 3 * ilv)[g.y0:g.y0 + g.rows]
    a = _filled(g, cells, poison, dev)
    stride, guard = g.width + 13, 256
    out = torch.full((guard + g.rows * stride + guard,), A5, dtype=torch.uint8, device=dev)
    s = g.strip()
    rc = lib.gol_strip_unpack(ctypes.byref(s), a.buf.data_ptr(), out.data_ptr() + guard, stride, value,
                              stream.cuda_stream)
    assert rc == 0, lib.gol_last_error()
    stream.synchronize()
    host = out.cpu().numpy()
    assert (host[:guard] == A5).all() and (host[guard + g.rows * stride:] == A5).all()
    body = host[guard:guard + g.rows * stride].reshape(g.rows, stride)
    np.testing.assert_array_equal(body[:, :g.width], cells * value)
    assert (body[:, g.width:] == A5).all()  # bytes from width to stride are the caller's
    _assert_untouched(a, None, "unpack source")


@pytest.mark.parametrize("poison", sa.POISONS)
@pytest.mark.parametrize("ilv,pad", LAYOUTS)
def test_strip_population_and_hash_see_the_owned_words_only(hip, oracle, ilv, pad, poison):
    eng, stream, dev, lib = hip
    for boundary in (sa.TORUS, sa.BOUNDED):
        geoms = _board_strips(ilv, boundary, pad)
        board = _board(geoms[0], 11 + ilv + boundary)
        acc = torch.zeros(8, dtype=torch.int64, device=dev)  # [1] population, [5] hash partial; the rest canaries
        arenas = []
        for g in geoms:
            a = _filled(g, board[g.y0:g.y0 + g.rows], poison, dev, seed=40 + g.y0)
            arenas.append(a)
            s = g.strip()
            assert lib.gol_strip_population(ctypes.byref(s), a.buf.data_ptr(), acc.data_ptr() + 8,
                                            stream.cuda_stream) == 0, lib.gol_last_error()
            assert lib.gol_strip_hash_partial(ctypes.byref(s), a.buf.data_ptr(), acc.data_ptr() + 40,
                                              stream.cuda_stream) == 0, lib.gol_last_error()
        stream.synchronize()
        host = acc.cpu().numpy()
        assert host[1] == int(board.sum())
        g = geoms[0]
        assert int(lib.gol_hash_finalize(int(host[5]) & (2**64 - 1), g.width, g.height)) == oracle.board_hash(board)
        assert not host[[0, 2, 3, 4, 6, 7]].any()
        for a in arenas:
            _assert_untouched(a, None, "reduction source")


def _view_counts(board, boundary, x, y, s, ow, oh):
    """numpy block sums of the view's cells (torus: wrapped; bounded: dead outside the board)."""
    h, w = board.shape
    ys, xs = y + np.arange(s * oh), x + np.arange(s * ow)
    if boundary == sa.TORUS:
        win = board[np.ix_(ys % h, xs % w)]
    else:
        win = np.zeros((s * oh, s * ow), np.uint8)
        yi, xi = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
        win[np.ix_(yi, xi)] = board[np.ix_(ys[yi], xs[xi])]
    return win.reshape(oh, s, ow, s).sum(axis=(1, 3)).astype(np.uint32)


@pytest.mark.parametrize("poison", sa.POISONS)
@pytest.mark.parametrize("ilv,pad", LAYOUTS)
def test_strip_view_counts_count_the_owned_rows_only(hip, ilv, pad, poison):
    """Scales on both sides of the streaming view kernel's cut-over (16 * ilv) and of its two-tile form (32 * ilv), so
    the per-pixel kernel and both streaming forms run (with 16-byte loads where the pitch is a multiple of 4 words,
    dword loads elsewhere); the strips add into one count buffer with canaries on both sides."""
    from gameoflifewithactors_amd import _lib

    eng, stream, dev, lib = hip
    for boundary in (sa.TORUS, sa.BOUNDED):
        geoms = _board_strips(ilv, boundary, pad, nblocks=10, rows=(56, 57, 55))
        g0 = geoms[0]
        board = _board(g0, 17 + ilv + boundary)
        arenas = [_filled(g, board[g.y0:g.y0 + g.rows], poison, dev, seed=50 + g.y0) for g in geoms]
        for scale in (3, 16 * ilv + 1, 32 * ilv, 40 * ilv):
            ow, oh = min(7, g0.width // scale), max(1, min(5, g0.height // scale))
            x, y = (37, g0.height - 9) if boundary == sa.TORUS else (-scale - 5, -7)
            guard = 64
            counts = torch.full((guard + ow * oh + guard,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            counts[guard:guard + ow * oh] = 0
            v = _lib.View(x, y, scale, ow, oh)
            for g, a in zip(geoms, arenas):
                s = g.strip()
                rc = lib.gol_strip_view_counts(ctypes.byref(s), a.buf.data_ptr(), ctypes.byref(v),
                                               counts.data_ptr() + 4 * guard, stream.cuda_stream)
                assert rc == 0, lib.gol_last_error()
            stream.synchronize()
            host = counts.cpu().numpy()
            assert (host[:guard] == 0x5A5A5A5A).all() and (host[guard + ow * oh:] == 0x5A5A5A5A).all(), (boundary, scale)
            np.testing.assert_array_equal(host[guard:guard + ow * oh].view(np.uint32).reshape(oh, ow),
                                          _view_counts(board, boundary, x, y, scale, ow, oh),
                                          err_msg=f"boundary={boundary} scale={scale}")
        for a in arenas:
            _assert_untouched(a, None, "view source")


# ---------------------------------------------------------------- host output canaries
TAIL = 4096  # bytes past the documented length of every host buffer, prefilled with 0xA5


def _canary(nbytes):
    return np.full(nbytes + TAIL, A5, np.uint8)


def _ptr(buf, ctype):
    return buf.ctypes.data_as(ctypes.POINTER(ctype))


def _tail_intact(buf, nbytes, what):
    assert (buf[nbytes:] == A5).all(), f"{what} wrote past its documented {nbytes} bytes"


@pytest.mark.parametrize("w,h,boundary,kw", [
    (100, 100, 0, {}),                      # a byte board
    (256, 96, 1, {}),                       # a packed board
    (512, 128, 0, {"devices": [0, 0]}),     # a multi-part board
])
def test_board_readbacks_stay_inside_their_host_buffers(gol, w, h, boundary, kw):
    """gol.h gives every host buffer's length; the bytes past it are the caller's."""
    from gameoflifewithactors_amd import _lib

    b0 = (np.random.default_rng(w + h).random((h, w)) < 0.4).astype(np.uint8)
    with gol.Board(w, h, boundary, **kw) as b:
        b.set_cells(b0).step(3)
        lib, hnd = b._lib, b._h
        cells = b.get_cells()

        x, y, rw, rh = 5, 7, w - 11, h - 13
        buf = _canary(rw * rh)
        assert lib.gol_get_region(hnd, x, y, rw, rh, _ptr(buf, ctypes.c_uint8)) == 0, lib.gol_last_error()
        np.testing.assert_array_equal(buf[:rw * rh].reshape(rh, rw), cells[y:y + rh, x:x + rw])
        _tail_intact(buf, rw * rh, "gol_get_region")

        stride = w + 29
        buf = _canary(stride * h)
        assert lib.gol_render_gray8(hnd, _ptr(buf, ctypes.c_uint8), stride, 200) == 0, lib.gol_last_error()
        frame = buf[:stride * h].reshape(h, stride)
        np.testing.assert_array_equal(frame[:, :w], cells * 200)
        assert not frame[:, w:].any()  # gol.h: the bytes between width and stride are set to 0
        _tail_intact(buf, stride * h, "gol_render_gray8")

        for scale, ow, oh in ((1, 9, 5), (3, 11, 7), (40, 2, 2)):
            v = _lib.View(3, 2, scale, ow, oh)
            want = b.view_counts(3, 2, scale, ow, oh)
            buf = _canary(4 * ow * oh)
            assert lib.gol_view_counts(hnd, ctypes.byref(v), _ptr(buf, ctypes.c_uint32)) == 0, lib.gol_last_error()
            np.testing.assert_array_equal(buf[:4 * ow * oh].view(np.uint32).reshape(oh, ow), want)
            _tail_intact(buf, 4 * ow * oh, "gol_view_counts")
            stride = ow + 5
            buf = _canary(stride * oh)
            assert lib.gol_render_view(hnd, ctypes.byref(v), 0, 255, _ptr(buf, ctypes.c_uint8), stride) == 0
            frame = buf[:stride * oh].reshape(oh, stride)
            np.testing.assert_array_equal(frame[:, :ow], np.where(want > 0, 255, 0))
            assert not frame[:, ow:].any()
            _tail_intact(buf, stride * oh, "gol_render_view")

        n = h * ((w + 63) // 64)
        buf = _canary(8 * n)
        assert lib.gol_save_packed(hnd, _ptr(buf, ctypes.c_uint64), n) == 0, lib.gol_last_error()
        np.testing.assert_array_equal(buf[:8 * n].view(np.uint64), b.save_packed().reshape(-1))
        _tail_intact(buf, 8 * n, "gol_save_packed")


def test_batch_readbacks_stay_inside_their_host_buffers(gol):
    w, h, count = 100, 100, 37
    with gol.BoardBatch(w, h, count) as b:
        b.seed_splitmix(5).step(3)
        lib, hnd = b._lib, b._h
        first, n = 3, 11
        want = b.get_cells(first, n)
        buf = _canary(n * w * h)
        assert lib.gol_batch_get_cells(hnd, first, n, _ptr(buf, ctypes.c_uint8), n * w * h) == 0, lib.gol_last_error()
        np.testing.assert_array_equal(buf[:n * w * h].reshape(n, h, w), want)
        _tail_intact(buf, n * w * h, "gol_batch_get_cells")

        buf = _canary(8 * count)
        assert lib.gol_batch_populations(hnd, _ptr(buf, ctypes.c_int64), count) == 0, lib.gol_last_error()
        np.testing.assert_array_equal(buf[:8 * count].view(np.int64), b.populations())
        _tail_intact(buf, 8 * count, "gol_batch_populations")

        buf = _canary(8 * count)
        assert lib.gol_batch_hashes(hnd, _ptr(buf, ctypes.c_uint64), count) == 0, lib.gol_last_error()
        np.testing.assert_array_equal(buf[:8 * count].view(np.uint64), b.hashes())
        _tail_intact(buf, 8 * count, "gol_batch_hashes")

        gens, every = 6, 2
        t = gens // every
        buf = _canary(4 * t * count)
        assert lib.gol_batch_step_trace(hnd, gens, every, _ptr(buf, ctypes.c_uint32), t * count) == 0, lib.gol_last_error()
        trace = buf[:4 * t * count].view(np.uint32).reshape(t, count)
        np.testing.assert_array_equal(trace[-1], b.populations())
        _tail_intact(buf, 4 * t * count, "gol_batch_step_trace")
