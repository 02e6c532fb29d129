"""The body of the sweep of the device-side window calls — gol_download_bits_window[_async],
gol_upload_bits_window, gol_digest_window / gol_digest_async, gol_density_window /
gol_density_async, gol_fill_random_window, gol_copy_window — over one board of one
storage kind, every call compared with the numpy model of tests/window_ops_model.py and
never with another call of the library.  Not collected: tests/test_gpu_window_ops.py
runs it on the GPU with stepping, tests/window_ops_cpu_check.py over the host-only HIP
stand-in without (its stencil launches do nothing; its fill, copy, packed-bit, digest
and density launchers run the row routines of the shared headers for all three storage
forms).  Windows, tiles, thresholds, shifts and copy sources all come from
window_ops_model, whose tables tests/test_window_ops_model.py pins on the CPU.

No comparison below sits in a `try`, and nothing is skipped: a pass that could prove
nothing (no live window, a dead or full board before a stepped comparison) fails."""
import ctypes

import numpy as np

import density_ref
import digest_ref
import window_ops_model as wm

EINVAL = -1
T0 = 0x66666666        # the starting soups: density 0.4
FULL = 1 << 32
SENT8, SENT32 = 0x5A, 0xA5A5A5A5


def u8p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def first_diff(a, b):
    if a.shape != b.shape:
        return f"shape {a.shape} want {b.shape}"
    bad = np.argwhere(a != b)
    return f"{len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def same(got, want, *what):
    assert got.shape == want.shape and (got == want).all(), (*what, first_diff(got, want))


def board_of(e, stepping, *what):
    """The board read back: the packed download, unpacked (its pad bits must be 0); on the GPU
    the byte download and the live count must agree with it."""
    cells = np.unpackbits(e.download_bits(), axis=1)
    assert not cells[:, e.cols:].any(), (*what, "a pad bit of download_bits is set")
    cells = cells[:, :e.cols]
    if stepping:
        same(e.download(), cells, *what, "download against download_bits")
        assert e.popcount() == int(cells.sum()), (*what, "popcount")
    return cells


def check_board(e, model, stepping, *what):
    same(board_of(e, stepping, *what), model, *what)


def whole(e):
    return (0, 0, e.rows, e.cols)


# ------------------------------------------------------------------ readers
def refused_density(e, w, tiles, tag):
    """col0 off a multiple of 32: GOL_EINVAL, and the caller's block is not written."""
    trows, tcols = density_ref.density_dims(w[2], w[3], *tiles)
    buf = np.full((trows, tcols), SENT32, np.uint32)
    rc = e.lib.gol_density_window(e._c, *w, *tiles, u32p(buf), tcols)
    assert rc == EINVAL and b"col0" in e.lib.gol_last_error(e._c), (tag, "density_window not refused", w, rc)
    assert (buf == SENT32).all(), (tag, "a refused density_window wrote counts", w)


def check_readers(e, model, wins, stepping, tag):
    """Every reader at every window against the model; returns the model after the generations
    that the async check stepped."""
    k, boundary, m = e.tblock_k, e.boundary, e.mesh_m
    live = dead = False
    eligible = 0
    for i, (_, *w) in enumerate(wins):
        want = wm.cut(model, w)
        live, dead = live or bool(want.any()), dead or not want.all()
        same(e.download_bits_window(*w), wm.bits(want), tag, "download_bits_window", w)
        tiles = wm.tile_plan(i)
        if wm.density_ok(w):
            same(e.density_window(*w, *tiles), wm.density(model, w, *tiles), tag, "density_window", w, tiles)
            if eligible % 8 == 0:   # the C ABI with ld > tcols: the slack elements stay as they were
                trows, tcols = density_ref.density_dims(w[2], w[3], *tiles)
                buf = np.full((trows, tcols + 2), SENT32, np.uint32)
                assert e.lib.gol_density_window(e._c, *w, *tiles, u32p(buf), tcols + 2) == 0, \
                    (tag, w, e.lib.gol_last_error(e._c))
                same(buf[:, :tcols], wm.density(model, w, *tiles), tag, "gol_density_window ld = tcols + 2", w, tiles)
                assert (buf[:, tcols:] == SENT32).all(), (tag, "density slack overwritten", w, tiles)
            eligible += 1
        else:
            refused_density(e, w, tiles, tag)
        # (after a refusal: the context still answers)
        assert e.digest_window(*w) == wm.digest(model, w), (tag, "digest_window", w)
        if i % 8 == 0:   # the C ABI with ld > row_bytes: slack bytes stay, pad bits are 0
            rb = (w[3] + 7) // 8
            buf = np.full((w[2], rb + 3), SENT8, np.uint8)
            assert e.lib.gol_download_bits_window(e._c, *w, u8p(buf), rb + 3) == 0, (tag, w, e.lib.gol_last_error(e._c))
            same(buf[:, :rb], wm.bits(want), tag, "gol_download_bits_window ld = row_bytes + 3", w)
            assert (buf[:, rb:] == SENT8).all(), (tag, "packed slack overwritten", w)
            assert not np.unpackbits(buf[:, :rb], axis=1)[:, w[3]:].any(), (tag, "a pad bit is set", w)
    assert live and dead, (tag, "no window with a live cell, or none with a dead one", live, dead)
    # digests of disjoint windows add: a tiling of the board, against the whole-board digest
    parts = []
    for w, _ in wm.tiling(wins, e.rows, e.cols):
        parts.append(e.digest_window(*w))
        assert parts[-1] == wm.digest(model, w), (tag, "digest_window of a tiling piece", w)
    assert digest_ref.add(*parts) == e.digest() == wm.digest(model, whole(e)), (tag, "digest of the tiling")
    # ... and every density map holds the board's live cells
    for tiles in wm.TILES:
        got = e.density(*tiles)
        same(got, wm.density(model, whole(e), *tiles), tag, "density", tiles)
        assert int(got.sum()) == int(model.sum()), (tag, "density map total", tiles)
    # async: the packed windows of one row class, a digest and a density map pending at once,
    # a step enqueued behind them, one sync: every result is the board before that step
    for cls in sorted({w[0] for w in wins}):
        ws = [w[1:] for w in wins if w[0] == cls]
        tiles = wm.tile_plan(cls)
        outs = [e.download_bits_window_async(*w) for w in ws]
        dg, dn = e.digest_async(), e.density_async(*tiles)
        wants = [wm.bits(wm.cut(model, w)) for w in ws]
        want_dg, want_dn = wm.digest(model, whole(e)), wm.density(model, whole(e), *tiles)
        if stepping:
            e.step(k)
        e.sync()
        for w, o, want in zip(ws, outs, wants):
            same(o, want, tag, "download_bits_window_async", w)
        assert (int(dg[0]), int(dg[1])) == want_dg, (tag, "digest_async", cls)
        same(dn, want_dn, tag, "density_async", cls, tiles)
        if stepping:
            model = wm.step(model, k, boundary, m)
    check_board(e, model, stepping, tag, "after the async pass")
    return model


# ------------------------------------------------------------------ writers
def fresh_cells(seed, w, cols):
    """A soup of density 0.5 for window w; a window that ends at the last column has its three
    rightmost columns all live (a live pad bit or ghost would change the next generation)."""
    row0, col0, nrows, ncols = w
    cells = wm.soup(seed, nrows, ncols, 0.5)
    if col0 + ncols == cols and ncols >= 3:
        cells[:, -3:] = 1
    return cells


def packed_with_pad_set(cells):
    """The packed rows of the cells with every pad bit set (upload ignores them)."""
    packed = wm.bits(cells)
    pad = 8 * packed.shape[1] - cells.shape[1]
    packed[:, -1] |= (1 << pad) - 1
    return packed


def put_fill(e, model, w, seed, T, stepping, tag):
    e.fill_random(window=tuple(w), seed=seed, threshold=T)
    wm.fill(model, w, seed, T, e.boundary)
    check_board(e, model, stepping, tag, "fill_random_window", w, seed, hex(T))


def put_bits(e, model, w, cells, stepping, tag, raw=False):
    packed = packed_with_pad_set(cells)
    if raw:   # the C ABI with strided rows whose slack is 0xFF
        rb = packed.shape[1]
        host = np.full((w[2], rb + 5), 0xFF, np.uint8)
        host[:, :rb] = packed
        assert e.lib.gol_upload_bits_window(e._c, *w, u8p(host), rb + 5) == 0, (tag, w, e.lib.gol_last_error(e._c))
    else:
        e.upload_bits_window(w[0], w[1], w[3], packed)
    wm.write(model, w[0], w[1], cells, e.boundary)
    check_board(e, model, stepping, tag, "upload_bits_window", "ld = row_bytes + 5" if raw else "", w)


def put_copy(e, model, w, src, smodel, sw, op, stepping, tag):
    e.copy_from(src, (sw[0], sw[1], w[2], w[3]), at=(w[0], w[1]), op=op)
    wm.merge(model, w, smodel, sw, op, e.boundary)
    check_board(e, model, stepping, tag, "copy_from", src.layout, src.tblock_k, src.boundary, w, sw, op)


def sources_unchanged(srcs, stepping, tag):
    for name, (src, smodel) in srcs.items():
        check_board(src, smodel, stepping, tag, "the copy source changed", name)


def serial_lines(e):
    """The corner, the last row, the last column and a 3 x 3 beside them."""
    rows, cols = e.rows, e.cols
    return ((rows - 3, cols - 3, 3, 3), (rows - 1, 0, 1, cols), (0, cols - 1, rows, 1), (rows - 4, cols - 4, 3, 3))


def dead_line_is_dead(e, stepping, tag, *what):
    got = board_of(e, stepping, tag, *what)
    assert not got[-1].any() and not got[:, -1].any(), (tag, "SERIAL_COMPAT's dead line written", *what)


def finish_pass(e, model, edge, stepping, tag, what):
    """The pass's writer at column 0, the last column (all rows) and one full row; then, with
    stepping, 2k + 1 generations against the model."""
    rows, cols = e.rows, e.cols
    for j, w in enumerate(((0, 0, rows, 1), (0, cols - 1, rows, 1), (rows // 2, 0, 1, cols))):
        edge(j, w)
    if not stepping:
        return model
    assert 0 < int(model.sum()) < model.size, (tag, what, "an empty or full board: the generations would prove nothing")
    gens = 2 * e.tblock_k + 1
    e.step(gens)
    model = wm.step(model, gens, e.boundary, e.mesh_m)
    assert model.any(), (tag, what, "the board died: nothing is compared")
    check_board(e, model, stepping, tag, what, f"{gens} generations on")
    return model


def fill_pass(e, model, order, stepping, tag):
    for i, (_, *w) in enumerate(order):
        put_fill(e, model, w, *wm.fill_plan(i), stepping, tag)
    if e.boundary == "serial_compat":
        for j, w in enumerate(serial_lines(e)):
            put_fill(e, model, w, 0x5E00 + j, FULL, stepping, tag)
            dead_line_is_dead(e, stepping, tag, "fill of ones", w)
    edge_t = (FULL, 1 << 31, 3 << 29)

    def edge(j, w):
        put_fill(e, model, w, 0xED00 + j, edge_t[j], stepping, tag)
    return finish_pass(e, model, edge, stepping, tag, "after the fills")


def bits_pass(e, model, order, stepping, tag):
    for i, (_, *w) in enumerate(order):
        put_bits(e, model, w, fresh_cells(3000 + i, w, e.cols), stepping, tag, raw=i % 8 == 1)
    if e.boundary == "serial_compat":
        for w in serial_lines(e):
            put_bits(e, model, w, np.ones((w[2], w[3]), np.uint8), stepping, tag)
            dead_line_is_dead(e, stepping, tag, "packed upload of ones", w)

    def edge(j, w):
        cells = np.ones((w[2], w[3]), np.uint8) if j == 0 else wm.soup(3900 + j, w[2], w[3], 0.5)
        put_bits(e, model, w, cells, stepping, tag, raw=j == 1)
    return finish_pass(e, model, edge, stepping, tag, "after the packed uploads")


def copy_pass(e, model, order, srcs, slabs, stepping, tag):
    rows, cols = e.rows, e.cols
    for i, ((_, *w), (names, srow0, scol0, op)) in enumerate(zip(order, wm.copy_plan(order, rows, cols, slabs))):
        for name in names:
            put_copy(e, model, w, *srcs[name], (srow0, scol0), op, stepping, tag)
        if i % 8 == 0:
            sources_unchanged(srcs, stepping, tag)
    sources_unchanged(srcs, stepping, tag)
    if e.boundary == "serial_compat":   # an all-ones source under every op
        ones, omodel = srcs["foreign"]
        ones.fill_random(seed=1, threshold=FULL)
        wm.fill(omodel, whole(ones), 1, FULL, ones.boundary)
        check_board(ones, omodel, stepping, tag, "the all-ones source")
        assert omodel.all()
        for w in serial_lines(e):
            for op in wm.OPS:
                put_copy(e, model, w, ones, omodel, w, op, stepping, tag)
                dead_line_is_dead(e, stepping, tag, "copy of ones", w, op)
    src, smodel = srcs["same"]
    edge_from = (((0, cols - 1), "replace"), ((0, 0), "xor"), ((rows // 2, 0), "or"))

    def edge(j, w):
        put_copy(e, model, w, src, smodel, *edge_from[j], stepping, tag)
    model = finish_pass(e, model, edge, stepping, tag, "after the copies")
    sources_unchanged(srcs, stepping, tag)
    return model


def make_source(gh, rows, cols, slabs, layout, k, boundary, m, seed, stepping, tag):
    """A copy source and its model: filled by seed and, with stepping, k generations on (its
    other buffer current, torus ghosts and halo rows as a step leaves them)."""
    e = gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, mesh_m=m, tblock_k=k)
    model = np.zeros((rows, cols), np.uint8)
    e.fill_random(seed=seed, threshold=T0)
    wm.fill(model, (0, 0, rows, cols), seed, T0, boundary)
    if stepping:
        e.step(k)
        model = wm.step(model, k, boundary, m)
    check_board(e, model, stepping, tag, "source", layout, k, boundary)
    assert 0 < int(model.sum()) < model.size, (tag, "source", layout, k, boundary)
    return e, model


def sweep(gh, kind, board, slabs, stepping):
    """One board of one kind in `slabs` slabs.  stepping: the step kernels compute (a GPU);
    without, the readers see the filled board once and no generation is compared."""
    layout, k, boundary = kind[:3]
    rows, cols, m = board
    ki = wm.KINDS.index(kind)
    tag = (layout, k, boundary, rows, cols, m, slabs)
    wins = wm.windows(rows, cols, wm.seams(rows), m)
    # the writers take the whole board and the corner cells first: the board that is stepped at the
    # end is then made of the list's windows, not of one whole-board write
    order = sorted(wins, key=lambda w: -w[0])
    flay, fk, fboundary = wm.foreign_kind(ki)
    s1, m1 = make_source(gh, rows, cols, slabs, layout, k, boundary, m, 0x51 + ki, stepping, tag)
    with s1:
        s2, m2 = make_source(gh, rows, cols, slabs, flay, fk, fboundary, 1, 0xF0 + ki, stepping, tag)
        with s2, gh.Engine(rows, cols, n_gpus=slabs, layout=layout, boundary=boundary, mesh_m=m, tblock_k=k) as e:
            srcs = {"same": (s1, m1), "foreign": (s2, m2)}
            if not stepping and (ki + slabs) % 2:
                e.step(k)   # the stand-in computes nothing, but the other (still empty) buffer is now current
            model = np.zeros((rows, cols), np.uint8)
            seed = rows * 1000 + cols + k
            e.fill_random(seed=seed, threshold=T0)
            wm.fill(model, whole(e), seed, T0, boundary)
            check_board(e, model, stepping, tag, "fill_random")
            if stepping:
                for s in (k, max(1, k - 3), 1):   # both ping-pong buffers and a short block are read
                    e.step(s)
                    model = wm.step(model, s, boundary, m)
                    model = check_readers(e, model, wins, stepping, tag + (e.generation,))
            else:
                model = check_readers(e, model, wins, stepping, tag + ("filled",))
            model = fill_pass(e, model, order, stepping, tag)
            model = bits_pass(e, model, order, stepping, tag)
            model = copy_pass(e, model, order, srcs, slabs, stepping, tag)
            check_readers(e, model, wins[::7] + [w for w in wins if w[1:] == whole(e)], stepping, tag + ("end",))
