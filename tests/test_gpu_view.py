"""GPU tests of the board view (gol_view_counts / gol_render_view / gol_strip_view_counts, csrc/gol_view.hip).

The reference everywhere is numpy on Board.get_cells() -- a path the rest of the suite pins to the oracle: index the
view's rows and columns (modulo the board on a torus, dead outside it when bounded), reshape to (out_h, s, out_w, s) and
sum.  Counts must be equal exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
SCALES = (1, 2, 3, 4, 5, 7, 31, 32, 33, 64, 127, 128, 129)


def ref_counts(cells, boundary, x, y, s, out_w, out_h):
    H, W = cells.shape
    ys, xs = y + np.arange(s * out_h, dtype=np.int64), x + np.arange(s * out_w, dtype=np.int64)
    if boundary == TORUS:
        sub = cells[np.ix_(ys % H, xs % W)]
    else:
        my, mx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        sub = np.zeros((ys.size, xs.size), dtype=np.uint8)
        sub[np.ix_(my, mx)] = cells[np.ix_(ys[my], xs[mx])]
    return (sub != 0).reshape(out_h, s, out_w, s).sum(axis=(1, 3), dtype=np.uint32)


def tone_np(counts, s, mode, alive):
    """gol_view_tone's formula on an array."""
    c = counts.astype(np.uint64)
    if mode == 0:
        return np.where(c > 0, alive, 0).astype(np.uint8)
    n = np.uint64(s * s)
    return ((np.uint64(2) * c * np.uint64(alive) + n) // (np.uint64(2) * n)).astype(np.uint8)


def make_board(w, h, boundary=TORUS, ilv=0, devices=None, seed=1, gens=7, options=None):
    from gameoflifewithactors_amd import Board

    b = Board(w, h, boundary, ilv=ilv, devices=devices, options=options)
    b.set_cells((np.random.default_rng(seed).random((h, w)) < 0.40).astype(np.uint8))
    if gens:
        b.step(gens)
    return b


# (width, height, ilv, devices): every packed layout on both sides of s = 32 ilv, 16-byte and odd pitches, three blocks,
# byte boards, and 30-row strips (s = 7 then puts tiles across strip boundaries)
LAYOUTS = [
    (256, 70, 1, None),
    (256, 70, 2, None),
    (512, 33, 4, None),
    (384, 50, 4, None),
    (96, 40, 0, None),
    (100, 100, 0, None),
    (257, 9, 0, None),
    (320, 90, 0, [0, 0, 0]),
    (512, 256, 4, None),  # tall enough for wide tiles at ilv 4 (s >= 128)
]


@pytest.mark.parametrize("w,h,ilv,devices", LAYOUTS)
def test_view_counts_layouts_and_scales(w, h, ilv, devices):
    with make_board(w, h, TORUS, ilv, devices, seed=w + h + ilv) as b:
        cells = b.get_cells()
        if devices:
            assert [p["rows"] for p in b.parts()] == [30, 30, 30]
        checked = 0
        for s in SCALES:
            if s > min(w, h):
                continue
            out_w, out_h = w // s, h // s
            for x, y in ((0, 0), (1, 5), (37 % w, h - 1), (w - 1, 0)):
                got = b.view_counts(x, y, s, out_w, out_h)
                want = ref_counts(cells, TORUS, x, y, s, out_w, out_h)
                assert got.dtype == np.uint32 and got.shape == (out_h, out_w)
                assert np.array_equal(got, want), (s, x, y, np.argwhere(got != want)[:4])
                checked += 1
        assert checked == 4 * sum(s <= min(w, h) for s in SCALES) >= 4 * 6


@pytest.mark.parametrize("w,h,ilv,devices", [(256, 70, 2, None), (100, 100, 0, None), (1024, 300, 0, [0, 0, 0, 0])])
def test_view_counts_bounded_overhang(w, h, ilv, devices):
    with make_board(w, h, BOUNDED, ilv, devices, seed=3 * w + h) as b:
        cells = b.get_cells()
        for s in (1, 2, 5, 33, 64, 65, 128):
            out_w, out_h = w // s + 2, h // s + 3  # past the board on every side the origin leaves room for
            for x, y in ((-3, -s), (w - s // 2, 0), (w - s // 2, h - 1), (-3 - s * out_w, 7), (w, 0), (0, h),
                         (2 ** 31, -(2 ** 31)), (-(2 ** 31), 2 ** 31)):
                got = b.view_counts(x, y, s, out_w, out_h)
                want = ref_counts(cells, BOUNDED, x, y, s, out_w, out_h)
                assert np.array_equal(got, want), (s, x, y)
                if x >= w or y >= h or x + s * out_w <= 0 or y + s * out_h <= 0:
                    assert not got.any()  # wholly outside the board: all dead


def test_view_stream_option_is_results_neutral():
    with make_board(512, 256, TORUS, 4, seed=11) as b:
        cells = b.get_cells()
        assert b.get_option("view_stream") == 1
        for s in (128, 129, 200):
            out_w, out_h = 512 // s, 256 // s
            for x, y in ((0, 0), (300, 255), (511, 130)):
                b.set_option("view_stream", 1)
                streamed = b.view_counts(x, y, s, out_w, out_h)
                b.set_option("view_stream", 0)
                assert b.get_option("view_stream") == 0
                per_pixel = b.view_counts(x, y, s, out_w, out_h)
                assert np.array_equal(streamed, per_pixel)
                assert np.array_equal(streamed, ref_counts(cells, TORUS, x, y, s, out_w, out_h))


@pytest.mark.parametrize("w,h,gens", [
    (1001, 300, 16),  # a ragged board whose state lives in its scratch words after the call
    (512, 512, 64),   # the rows-on-lanes pass
    (100, 100, 100),  # the single-wave pass
])
def test_view_sees_the_current_generation(w, h, gens):
    """The view is taken BEFORE any other readback: it must bring a ragged board's bytes up to date itself."""
    with make_board(w, h, TORUS, seed=gens, gens=0) as b:
        b.step(gens)
        s = 7
        got = b.view_counts(w - 3, h - 2, s, w // s, h // s)
        cells = b.get_cells()
        assert np.array_equal(got, ref_counts(cells, TORUS, w - 3, h - 2, s, w // s, h // s))
        assert b.generation == gens


@pytest.mark.parametrize("w,h,ilv,devices", [(256, 70, 2, None), (100, 100, 0, None), (320, 90, 0, [0, 0, 0])])
def test_view_identities(w, h, ilv, devices):
    from gameoflifewithactors_amd import VIEW_ANY, VIEW_DENSITY, view_tone

    with make_board(w, h, TORUS, ilv, devices, seed=5) as b:
        gen, digest = b.generation, b.hash()
        # scale 1 over the whole board is the Gray8 frame, in either mode, padding included
        frame = b.render_gray8(128, stride=w + 3).reshape(h, w + 3)
        for mode in (VIEW_ANY, VIEW_DENSITY):
            got = b.render_view(0, 0, 1, w, h, mode, 128, stride=w + 3)
            assert got.shape == (h, w + 3) and np.array_equal(got, frame)
        # a whole-board view holds every live cell once
        s = 5 if w % 5 == 0 else 2
        assert int(b.view_counts(0, 0, s, w // s, h // s).sum(dtype=np.uint64)) == b.population()
        assert int(b.view_counts(w - 1, h - 1, 1, w, h).sum(dtype=np.uint64)) == b.population()
        # the frame is the tone map of the counts, element by element
        for s, mode, alive in ((3, VIEW_DENSITY, 255), (3, VIEW_ANY, 200), (33, VIEW_DENSITY, 128), (1, VIEW_DENSITY, 7)):
            out_w, out_h = w // s, h // s
            counts = b.view_counts(2, 1, s, out_w, out_h)
            pixels = b.render_view(2, 1, s, out_w, out_h, mode, alive)
            want = np.array([[view_tone(int(c), s, mode, alive) for c in row] for row in counts], dtype=np.uint8)
            assert pixels.shape == (out_h, out_w) and np.array_equal(pixels, want)
            assert np.array_equal(pixels, tone_np(counts, s, mode, alive))
        # a view changes nothing
        assert b.generation == gen and b.hash() == digest


def test_view_rejects_bad_arguments():
    with make_board(256, 70, TORUS, 2, gens=0) as b:
        for bad in ((0, 0, 0, 4, 4), (0, 0, 32769, 1, 1), (0, 0, 1, 0, 4), (0, 0, 4, 65, 4), (256, 0, 1, 4, 4),
                    (0, 70, 1, 4, 4), (0, 0, 2, 4, 36)):
            with pytest.raises(ValueError):
                b.view_counts(*bad)
        with pytest.raises(ValueError):
            b.render_view(0, 0, 1, 8, 8, mode=2)
        with pytest.raises(ValueError):
            b.render_view(0, 0, 1, 8, 8, stride=7)


@pytest.mark.parametrize("mode", [0, 1])
def test_driver_emits_view_frames(mode):
    from gameoflifewithactors_amd.driver import UpdateAgent, run
    from gameoflifewithactors_amd.logic import Grid

    g, view = Grid(256, 256), (0, 0, 4, 64, 64)
    frames, twin_frames = [], []
    with run(g, seed=42, emit="view", view=view, view_mode=mode,
             agent=UpdateAgent(g, 128, on_frame=lambda p: frames.append(np.array(p)))) as game, \
            run(g, seed=42, emit="pixels",
                agent=UpdateAgent(g, 128, on_frame=lambda p: twin_frames.append(np.array(p)))) as twin:
        for _ in range(3):
            game.update_view()
            twin.update_view()
    assert len(frames) == 3 and len(twin_frames) == 3
    for f, t in zip(frames, twin_frames):
        assert f.shape == (64 * 64,) and f.dtype == np.uint8
        cells = (t.reshape(256, 256) != 0).astype(np.uint8)
        assert cells.any()
        want = tone_np(ref_counts(cells, TORUS, *view), 4, mode, 128)
        assert np.array_equal(f.reshape(64, 64), want)
    with pytest.raises(ValueError):
        run(g, seed=1, emit="view")


def test_strip_primitive_counts_owned_rows_only():
    """Two strips of a 256 x 64 torus with 8 ghost rows each, the ghost rows full of live cells: both calls added
    into one zeroed tensor give the board's counts; a primitive that counted ghost rows would not."""
    from gameoflifewithactors_amd.strips import Geometry, HipEngine

    dev = torch.device("cuda", 0)
    w, h, ghost, ilv = 256, 64, 8, 2
    cells = (np.random.default_rng(8).random((h, w)) < 0.40).astype(np.uint8)
    stream = torch.cuda.Stream(dev)
    with HipEngine(dev) as eng:
        strips = []
        for y0 in (0, 32):
            geom = Geometry(w, h, y0, 32, ghost, w // 32, TORUS, False, ilv)
            buf = eng.alloc(geom, stream)
            eng.set_cells(geom, buf, torch.from_numpy(cells[y0:y0 + 32]), stream)
            with torch.cuda.stream(stream):
                buf[:ghost].fill_(-1)
                buf[ghost + 32:].fill_(-1)
            strips.append((geom, buf))
        for view in ((0, 0, 1, w, h), (3, 29, 7, 36, 9), (250, 40, 33, 7, 1), (10, 5, 64, 4, 1), (0, 0, 16, 16, 4)):
            x, y, s, out_w, out_h = view
            with torch.cuda.stream(stream):
                counts = torch.zeros(out_h * out_w, dtype=torch.int32, device=dev)
            for geom, buf in strips:
                eng.view_counts(geom, buf, view, counts, stream)
            stream.synchronize()
            got = counts.cpu().numpy().astype(np.uint32).reshape(out_h, out_w)
            assert np.array_equal(got, ref_counts(cells, TORUS, x, y, s, out_w, out_h)), view


def test_view_offsets_past_4gib():
    """A 262144 x 131200 torus: its buffer is 128 rows longer than 2^32 bytes, so the last rows are reached only with
    64-bit offsets.  scale * out_h <= height on a torus and 131200 = 32 * 4096 + 128, so the whole board is the
    s = 4096 view of the first 131072 rows plus an s = 128 view of the 128 rows past them (all beyond 2^32 bytes);
    together they must hold every live cell once."""
    from gameoflifewithactors_amd import Board

    free, _total = torch.cuda.mem_get_info(0)
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    w, h = 262144, 131200
    with Board(w, h) as b:
        assert b.info()["pitch"] * 4 * h > 2 ** 32
        b.seed_splitmix(1)
        pop = b.population()
        low = b.view_counts(0, 0, 4096, w // 4096, 32)
        high = b.view_counts(0, 32 * 4096, 128, w // 128, 1)
        assert high.any()
        assert int(low.sum(dtype=np.uint64)) + int(high.sum(dtype=np.uint64)) == pop
        # the s = 4096 view wrapped so that one tile row holds the rows past 2^32 bytes
        wrapped = b.view_counts(0, h - 4096, 4096, w // 4096, 32)
        assert int(wrapped.sum(dtype=np.uint64)) + int(b.view_counts(0, h - 4096 - 128, 128, w // 128, 1).sum(
            dtype=np.uint64)) == pop
        tiles = b.view_counts(0, h - 512, 512, w // 512, 1)
        for i in (0, 255, 511):
            assert int(tiles[0, i]) == int(b.get_region(512 * i, h - 512, 512, 512).sum(dtype=np.uint64)), i
