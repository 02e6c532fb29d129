"""The byte-window and snapshot-text calls — gol_upload_window, gol_download_window,
gol_download_window_async, gol_format_text, gol_parse_text — swept over every storage
form and column alignment against one numpy model of the logical board
(tests/window_model.py, pinned on the CPU by tests/test_window_model.py).

Per storage kind (layout x group width x boundary, 1 and 3 slabs): a soup is uploaded
and stepped [k, max(1, k - 3), 1]; after each step every reader is compared with the
model at every window of the list (both window edges in every residue class mod 32,
1-cell, 1-row and 1-column windows, windows across slab seams, mesh block seams, the
last row and column), async windows a row class at a time with a step enqueued behind
them, the text at two block sizes, the C ABI with ld > ncols.  Then every writer
replaces every window with a fresh soup — through the binding, through text, and
through the C ABI with strided rows and with live cells spelled 2, 0x80 and 0xFF —
and the whole board, its popcount and the generations that follow must be the
model's: a stale torus ghost, a live pad bit, a live cell in SERIAL_COMPAT's dead
line or a halo row left behind at a slab seam changes those generations.

What a defect in these paths would turn red first (read from the code; windows are
(row0, col0, nrows, ncols), all in test_window_io_sweep):
  `c >= col0 + ncols` as `>` in pack_window_kernel   bit-k3-dead, upload_window (13, 0, 5, 2): column 2
                                                      takes the first cell of the window's next row
  bit_word / bit_pos at the wrong group width         bit-k8-dead, the download after the first upload
  enforce_inactive skipped on the byte layout         byte-k2-serial_compat, the first upload (a live last
                                                      column); then the all-ones window (34, 34, 3, 3)
  `c < active_cols` dropped from the pack kernel      bit-k2-serial_compat, the same two
  wrap_rows skipped at the end of upload_piece        bit-k3-torus, download_window (0, 0, 40, 1) after the
                                                      first 3 generations (ghosts still zero)
  a mesh run at the logical, not the storage column   bit-k2-mesh_compat 96 / m = 3: the first upload where one
                                                      side is wrong, the first 2 generations where all are
                                                      (then the board is stepped with its blocks unreversed)
  w.ld as w.ncols at the delivery of a window         bit-k3-dead, gol_download_window_async (0, 0, 40, 1) at
                                                      ld = 8: rows land 1 byte apart, the 0x5A slack is written
  launch_normalize_bytes removed                      byte-k1-dead, gol_upload_window of 2 / 0x80 / 0xFF at
                                                      (39, 1, 1, 31): the download returns 0x80
  a text block seam dropping or repeating a byte      every kind, format_text (0, 0, 40, 300) at 1000-byte
                                                      blocks: 40 blocks of one row, 3 slabs"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_model as wm  # noqa: E402

TEXT_BLOCK_DEFAULT = 64 << 20
SPELLINGS = np.array([2, 0x80, 0xFF, 1], np.uint8)   # a live cell, as a caller's bool array may hold it


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


def u8p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def first_diff(a, b):
    if a.shape != b.shape:
        return f"shape {a.shape} want {b.shape}"
    bad = np.argwhere(a != b)
    return f"{len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def cut(model, w):
    row0, col0, nrows, ncols = w
    return model[row0:row0 + nrows, col0:col0 + ncols]


def same(got, want, *what):
    assert got.shape == want.shape and (got == want).all(), (*what, first_diff(got, want))


# ------------------------------------------------------------------ readers
def check_readers(gh, e, model, wins, tag):
    """Every reader against the model; returns the model after the generations the async check stepped."""
    k, boundary, m = e.tblock_k, e.boundary, e.mesh_m
    for i, (_, *w) in enumerate(wins):
        same(e.download_window(*w), cut(model, w), tag, "download_window", w)
        if i % 10 == 0:   # the old path against the packed one
            same(np.packbits(e.download_window(*w), axis=1), e.download_bits_window(*w), tag, "bits", w)
    # text, at the default block size and in blocks that hold one or two rows of the wide windows
    for block in (TEXT_BLOCK_DEFAULT, 1000):
        e.set_option(gh.OPT_TEXT_BLOCK_BYTES, block)
        for _, *w in wins:
            got, want = e.format_text(*w), wm.text(cut(model, w))
            assert got == want, (tag, "format_text", block, w, len(got), len(want),
                                 next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), None))
    e.set_option(gh.OPT_TEXT_BLOCK_BYTES, TEXT_BLOCK_DEFAULT)
    # the C ABI with ld > ncols: bytes [ncols, ld) of every row stay as they were
    for i, (_, *w) in enumerate(wins):
        if i % 8:
            continue
        nrows, ncols = w[2], w[3]
        ld = ncols + (7 if i % 16 == 0 else 1)
        for call in (e.lib.gol_download_window, e.lib.gol_download_window_async):
            buf = np.full((nrows, ld), 0x5A, np.uint8)
            assert call(e._c, *w, u8p(buf), ld) == 0, (tag, w, e.lib.gol_last_error(e._c))
            e.sync()
            same(buf[:, :ncols], cut(model, w), tag, call.__name__, "ld", ld, w)
            assert (buf[:, ncols:] == 0x5A).all(), (tag, call.__name__, "slack overwritten", ld, w)
    # async: the windows of one row class pending at once, a step enqueued behind them, one sync
    seen_live = False
    for cls in sorted({w[0] for w in wins}):
        ws = [w[1:] for w in wins if w[0] == cls]
        outs = [e.download_window_async(*w) for w in ws]
        wants = [cut(model, w).copy() for w in ws]
        e.step(k)
        e.sync()
        for w, o, want in zip(ws, outs, wants):
            same(o, want, tag, "download_window_async", w)
            seen_live = seen_live or bool(want.any())
        model = wm.step(model, k, boundary, m)
    assert seen_live, tag
    same(e.download(), model, tag, "after the async steps")
    return model


# ------------------------------------------------------------------ writers
def check_board(e, model, *what):
    same(e.download(), model, *what)
    assert e.popcount() == int(model.sum()), what


def fresh_cells(seed, w, cols):
    """A soup of density 0.5 for window w; a window that ends at the last column has its three
    rightmost columns all live (a live pad bit or ghost would change the next generation)."""
    row0, col0, nrows, ncols = w
    cells = wm.soup(seed, nrows, ncols, 0.5)
    if col0 + ncols == cols and ncols >= 3:
        cells[:, -3:] = 1
    return cells


def raw_upload(e, w, host, ld, tag):
    assert host.flags["C_CONTIGUOUS"] and host.shape == (w[2], ld)
    assert e.lib.gol_upload_window(e._c, *w, u8p(host), ld) == 0, (tag, w, e.lib.gol_last_error(e._c))


def write_upload_window(gh, e, model, wins, tag):
    """upload_window of a fresh soup at every window: only the window changes."""
    for i, (_, *w) in enumerate(wins):
        cells = fresh_cells(1000 + i, w, e.cols)
        e.upload_window(w[0], w[1], cells)
        wm.write(model, w[0], w[1], cells, e.boundary)
        check_board(e, model, tag, "upload_window", w)


def write_text_and_raw(gh, e, model, wins, tag):
    """parse_text at every third window; the C ABI with strided rows whose slack is 0xFF, and with
    live cells spelled 2, 0x80 and 0xFF, at every eighth."""
    for i, (_, *w) in enumerate(wins):
        row0, col0, nrows, ncols = w
        if i % 3 == 0:
            cells = fresh_cells(5000 + i, w, e.cols)
            e.set_option(gh.OPT_TEXT_BLOCK_BYTES, 1000 if i % 6 else TEXT_BLOCK_DEFAULT)
            e.parse_text(*w, wm.text(cells))
            wm.write(model, row0, col0, cells, e.boundary)
            check_board(e, model, tag, "parse_text", w)
        if i % 8 == 1:
            cells = fresh_cells(7000 + i, w, e.cols)
            host = np.full((nrows, ncols + 7), 0xFF, np.uint8)
            host[:, :ncols] = cells
            raw_upload(e, w, host, ncols + 7, tag)
            wm.write(model, row0, col0, cells, e.boundary)
            check_board(e, model, tag, "gol_upload_window ld = ncols + 7", w)
        if i % 8 == 5:
            cells = fresh_cells(9000 + i, w, e.cols)
            rr, cc = np.indices(cells.shape)
            host = np.ascontiguousarray(cells * SPELLINGS[(rr + 2 * cc + i) % 4])
            assert set(np.unique(host)) <= {0, 1, 2, 0x80, 0xFF} and ((host != 0) == (cells != 0)).all()
            raw_upload(e, w, host, ncols, tag)
            wm.write(model, row0, col0, host, e.boundary)
            check_board(e, model, tag, "gol_upload_window of 2 / 0x80 / 0xFF", w)
            same(e.download_window(*w), cut(model, w), tag, "download_window of 2 / 0x80 / 0xFF", w)
    e.set_option(gh.OPT_TEXT_BLOCK_BYTES, TEXT_BLOCK_DEFAULT)
    # every spelling over the whole first and last column and a row across both slab seams' columns
    for j, w in enumerate(((0, 0, e.rows, 1), (0, e.cols - 1, e.rows, 1), (e.rows // 2, 0, 1, e.cols))):
        host = np.full((w[2], w[3]), SPELLINGS[j], np.uint8)
        raw_upload(e, w, host, w[3], tag)
        wm.write(model, w[0], w[1], host, e.boundary)
        check_board(e, model, tag, "a line of", int(SPELLINGS[j]), w)


def write_serial_dead_line(e, model, tag):
    """SERIAL_COMPAT: all-ones windows over the corner, the last row and the last column leave the
    dead row and column dead; so does a window beside them."""
    rows, cols = e.rows, e.cols
    for w in ((rows - 3, cols - 3, 3, 3), (rows - 1, 0, 1, cols), (0, cols - 1, rows, 1), (rows - 4, cols - 4, 3, 3),
              (0, 0, rows, cols)):
        ones = np.ones((w[2], w[3]), np.uint8)
        e.upload_window(w[0], w[1], ones)
        wm.write(model, w[0], w[1], ones, "serial_compat")
        got = e.download()
        assert not got[-1].any() and not got[:, -1].any(), (tag, "dead line written", w)
        check_board(e, model, tag, "all-ones window", w)
        e.parse_text(*w, wm.text(ones))
        check_board(e, model, tag, "all-ones text", w)
    assert int(model.sum()) == (rows - 1) * (cols - 1)
    cells = wm.soup(77, rows, cols, 0.5)    # ... and back to a board worth stepping
    e.upload_window(0, 0, cells)
    wm.write(model, 0, 0, cells, "serial_compat")
    check_board(e, model, tag, "soup over the ones")


def step_and_compare(e, model, tag, what):
    gens = 2 * e.tblock_k + 1
    e.step(gens)
    model = wm.step(model, gens, e.boundary, e.mesh_m)
    assert model.any(), (tag, what, "the board died: nothing is compared")
    check_board(e, model, tag, what, f"{gens} generations on")
    return model


def sweep(gh, layout, k, boundary, rows, cols, m, slabs):
    tag = (layout, k, boundary, rows, cols, m, slabs)
    wins = wm.windows(rows, cols, wm.seams(rows), m)
    # the writers take the whole board and the corner cells first: the board that is stepped at the
    # end is then made of the list's windows, not of one whole-board write
    order = sorted(wins, key=lambda w: -w[0])
    model = wm.soup(rows * 1000 + cols + k, rows, cols, 0.4)
    with gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, mesh_m=m, tblock_k=k) as e:
        e.upload(model)
        wm.write(model, 0, 0, model.copy(), boundary)
        check_board(e, model, tag, "upload")
        for s in (k, max(1, k - 3), 1):   # both ping-pong buffers and a short block are read
            e.step(s)
            model = wm.step(model, s, boundary, m)
            model = check_readers(gh, e, model, wins, tag + (e.generation,))
        write_upload_window(gh, e, model, order, tag)
        model = step_and_compare(e, model, tag, "after the window uploads")
        write_text_and_raw(gh, e, model, order, tag)
        if boundary == "serial_compat":
            write_serial_dead_line(e, model, tag)
        model = step_and_compare(e, model, tag, "after the last write")
        check_readers(gh, e, model, wins[::7] + [w for w in wins if w[1:] == (0, 0, rows, cols)], tag + ("end",))


@pytest.mark.parametrize("kind", wm.KINDS, ids=wm.kind_id)
def test_window_io_sweep(gh, kind):
    layout, k, boundary, boards = kind
    for rows, cols, m in boards:
        for slabs in wm.slab_counts(rows, k):
            sweep(gh, layout, k, boundary, rows, cols, m, slabs)


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("layout", ["bit", "byte"])
def test_ld_below_ncols_is_refused(gh, layout):
    b = wm.soup(2, 20, 100)
    with gh.Engine(20, 100, layout=layout, n_gpus=2, tblock_k=2) as e:
        e.upload(b)
        buf = np.full((6, 40), 0x5A, np.uint8)
        for call in (e.lib.gol_download_window, e.lib.gol_download_window_async, e.lib.gol_upload_window):
            for ld in (39, 1, 0, -40):
                assert call(e._c, 7, 33, 6, 40, u8p(buf), ld) == -1, (call.__name__, ld)
                assert b"ld < ncols" in e.lib.gol_last_error(e._c)
        e.sync()
        assert (buf == 0x5A).all()
        same(e.download(), b, layout, "after the refused calls")
        e.step(3)
        from oracle import golcpu as g
        same(e.download(), g.run(b, 3, g.DEAD), layout, "a step after the refused calls")
