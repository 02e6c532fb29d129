"""RLE pattern text on the GPU (gol_format_rle / gol_rle_bytes / gol_write_rle /
gol_parse_rle / gol_read_rle).  The master property: in every state of every context
format_rle(window) equals rle_ref.encode(download_window(window)) byte for byte, and
parsing that text into a context of another kind that was filled with ones gives the
window back and changes no cell outside its box — every layout and group width, a
torus, MESH_COMPAT's column runs, SERIAL_COMPAT, slabs and rank contexts; hand-built
rows (runs of 1 .. 1000, the word, span and pass seams, leading and inner empty rows,
the all-dead window), rows of two workgroup passes + 33 columns, blocks of 1 and 3
rows against the one-block text, the Gosper gun against the CPU oracle, the rule in
the header, GOL_ESTATE under the clock probe, and bin/gol --format rle / --pattern."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
EXE = os.path.join(ROOT, "mpi_amd", "bin", "gol")
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")

import rle_ref  # noqa: E402

KINDS = [("bit", 1), ("bit", 7), ("bit", 8), ("bit", 16), ("byte", 1), ("byte", 16)]
WINDOWS = [None, (3, 1, 64, 131), (0, 0, 1, 1), (5, 37, 9, 96)]
GUN_BODY = b"24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$10bo5bo7bo$11bo3bo$12b2o!\n"
GUN = b"x = 36, y = 9, rule = B3/S23\n" + GUN_BODY


@pytest.fixture(scope="module")
def gh():
    from mpi_amd import golhip
    golhip.load()
    return golhip


@pytest.fixture(scope="module")
def g():
    from oracle import golcpu
    return golcpu


def soup(seed, rows, cols, p=0.4):
    return (np.random.default_rng(seed).random((rows, cols)) < p).astype(np.uint8)


def block_steps(k):
    return [k, max(1, k - 3), 1, k]


def master(e, e2, windows, what):
    """format_rle == encode(download_window); parsed into e2 (filled with ones) the box is the window, the rest ones."""
    for win in windows:
        r0, c0, nr, nc = win or (0, 0, e.rows, e.cols)
        cells = e.download_window(r0, c0, nr, nc)
        want = rle_ref.encode(cells, *e.rule)
        got = e.format_rle(win)
        assert got == want, (what, win, got[:120], want[:120])
        assert e.rle_bytes(win) == len(want), (what, win)
        ones = np.ones((e2.rows, e2.cols), np.uint8)
        e2.upload(ones)
        at = (min(2, e2.rows - nr), min(3, e2.cols - nc))
        assert e2.parse_rle(got, at=at) == (nc, nr)
        ones[at[0]:at[0] + nr, at[1]:at[1] + nc] = cells
        back = e2.download()
        assert (back == ones).all(), (what, win, np.argwhere(back != ones)[:3])


# ------------------------------------------------------------------ the master property
@pytest.mark.parametrize("i", range(len(KINDS)))
def test_master_property_on_every_kind(gh, i):
    (layout, k), (layout2, k2) = KINDS[i], KINDS[(i + 1) % len(KINDS)]
    rows, cols = 70, 200
    with gh.Engine(rows, cols, layout=layout, tblock_k=k) as e, gh.Engine(rows, cols, layout=layout2, tblock_k=k2) as e2:
        e.upload(soup(3 + i, rows, cols))
        master(e, e2, WINDOWS, (layout, k, "initial"))
        for st in block_steps(k):
            e.step(st)
        assert e.popcount() > 0
        master(e, e2, WINDOWS, (layout, k, "stepped"))
        assert e.generation == sum(block_steps(k)) and e2.generation == 0


@pytest.mark.parametrize("kw,rows,cols", [(dict(layout="bit", boundary="torus", tblock_k=8), 70, 200),
                                          (dict(layout="byte", boundary="torus", tblock_k=8), 70, 200),
                                          (dict(layout="bit", boundary="mesh_compat", mesh_m=2), 128, 128),
                                          (dict(layout="byte", boundary="mesh_compat", mesh_m=2), 72, 72),
                                          (dict(layout="bit", boundary="serial_compat", tblock_k=4), 70, 70),
                                          (dict(layout="bit", tblock_k=2, n_gpus=3), 70, 200),
                                          (dict(layout="byte", tblock_k=8, n_gpus=3), 70, 200)])
def test_master_property_on_boundaries_and_slabs(gh, kw, rows, cols):
    wins = [None, (3, 1, 60, cols - 3), (5, 37, 9, cols - 40)]   # (across both seams of three slabs)
    with gh.Engine(rows, cols, **kw) as e, gh.Engine(rows, cols, layout="bit", tblock_k=1) as e2:
        e.upload(soup(9, rows, cols))
        master(e, e2, wins, (kw, "initial"))
        e.step(2 * kw.get("tblock_k", 1) + 1)
        master(e, e2, wins, (kw, "stepped"))
    # ... and read into such a context: the box is replaced, ghosts and the inactive region follow
    b = soup(10, rows, cols)
    with gh.Engine(rows, cols, layout="byte", tblock_k=1) as src, gh.Engine(rows, cols, **kw) as e, \
            gh.Engine(rows, cols, **kw) as twin:
        src.upload(b)
        e.upload(np.ones((rows, cols), np.uint8))
        base = e.download()   # (SERIAL_COMPAT keeps its last row and column dead)
        win = (3, 1, 60, cols - 3)
        assert e.parse_rle(src.format_rle(win), at=(3, 1)) == (cols - 3, 60)
        base[3:63, 1:cols - 2] = b[3:63, 1:cols - 2]
        if kw.get("boundary") == "serial_compat":
            base[-1] = 0
            base[:, -1] = 0
        assert (e.download() == base).all(), kw
        twin.upload(base)
        st = 2 * kw.get("tblock_k", 1) + 1
        e.step(st)
        twin.step(st)
        assert (e.download() == twin.download()).all(), kw


def test_rank_contexts(gh):
    assert os.path.exists(SHIM), "build the shim first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rle_rank_check.py"), SHIM],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rle ranks ok" in r.stdout


# ------------------------------------------------------------------ hand-built rows
def hand_board():
    b = np.zeros((40, 2100), np.uint8)
    c = 3
    for n in (1, 2, 9, 10, 99, 100, 999):   # rows 0..2 stay empty: a leading 3$
        b[3, c:c + n] = 1
        c += n + 2
    b[4, 5:1005] = 1
    for seam in (32, 64, 128, 2048):
        b[5, seam - 1:seam + 1] = 1
    b[6, :7] = 1            # live from column 0
    b[7, 2099] = 1          # live only in its last column
    b[8, :] = 1             # all live
    b[10, 500:503] = 1      # a gap of 1 empty row
    b[13, 31] = 1           # 2
    b[24, :33] = 1          # 10
    b[36, 2047:2100] = 1    # 11
    b[39, 2099] = 1         # the last row and column
    return b


HAND_WINDOWS = [None, (8, 0, 1, 32), (8, 0, 1, 64), (8, 0, 1, 33), (8, 0, 1, 1), (0, 0, 3, 64), (3, 0, 2, 2100),
                (5, 31, 9, 96), (20, 2040, 20, 60), (9, 0, 1, 2100), (7, 2068, 1, 32)]


def test_hand_built_rows(gh):
    b = hand_board()
    with gh.Engine(40, 2100, layout="bit", tblock_k=1) as e, gh.Engine(40, 2100, layout="byte", tblock_k=1) as e2:
        e.upload(b)
        assert e.format_rle().startswith(b"x = 2100, y = 40, rule = B3/S23\n3$3bo2b2o2b9o2b10o2b99o2b100o2b\n999o$5b1000o$31b2o")
        assert e.format_rle((0, 0, 3, 64)) == b"x = 64, y = 3, rule = B3/S23\n!\n"
        assert e.format_rle((8, 0, 1, 32)) == b"x = 32, y = 1, rule = B3/S23\n32o!\n"
        assert e.format_rle((20, 2040, 20, 60)) == b"x = 60, y = 20, rule = B3/S23\n16$7b53o3$59bo!\n"
        master(e, e2, HAND_WINDOWS, "hand")


@pytest.mark.parametrize("block", [1, None])
def test_blocks_give_the_one_block_text(gh, block):
    """GOL_OPT_TEXT_BLOCK_BYTES = 1: one row per block; the other value: three rows per block."""
    b = hand_board()
    with gh.Engine(40, 2100, layout="bit", tblock_k=1, n_gpus=2) as e, gh.Engine(40, 2100, layout="bit", tblock_k=8) as e2:
        e.upload(b)
        whole = {w: e.format_rle(w) for w in HAND_WINDOWS}
        assert whole[None] == rle_ref.encode(b)
        # worst-case bytes of a row of 2100 cells: 2100 + 1 + 4 + 2101 / 14 + 1 = 2256
        e.set_option(gh.OPT_TEXT_BLOCK_BYTES, block or 3 * 2256 + 100)
        e2.set_option(gh.OPT_TEXT_BLOCK_BYTES, block or 3 * 264)   # (reading: rows of 264 packed bytes)
        for w in HAND_WINDOWS:
            assert e.format_rle(w) == whole[w], (block, w)
            assert e.rle_bytes(w) == len(whole[w]), (block, w)
        e2.upload(np.ones((40, 2100), np.uint8))
        assert e2.parse_rle(whole[None]) == (2100, 40)
        assert (e2.download() == b).all()


# ------------------------------------------------------------------ long rows
def test_long_rows(gh):
    cols = 2 * 32768 + 33
    b = np.zeros((3, cols), np.uint8)
    b[0] = soup(5, 1, cols, 0.5)[0]
    b[1, 32760:32776] = 1
    b[2, 0] = b[2, cols - 1] = 1
    want = rle_ref.encode(b)
    with gh.Engine(3, cols, layout="bit", tblock_k=1) as e, gh.Engine(3, cols, layout="byte", tblock_k=1) as e2:
        e.upload(b)
        got = e.format_rle()
        assert got == want, [i for i in range(min(len(got), len(want))) if got[i] != want[i]][:3]
        assert got.replace(b"\n", b"").endswith(b"$32760b16o$o65567bo!") and e.rle_bytes() == len(want)
        assert e.format_rle((1, 0, 2, 32768 + 8)) == rle_ref.encode(b[1:3, :32776])   # a run up to the last column
        e2.upload(np.ones((3, cols), np.uint8))
        assert e2.parse_rle(got) == (cols, 3)
        assert (e2.download() == b).all()


# ------------------------------------------------------------------ a real pattern
def test_gosper_gun_against_the_oracle(gh, g, tmp_path):
    """The issue's gun file has its 98-character body on one line, which the format's own line rule
    (a newline after every 23rd token for a 9 x 36 window) breaks twice: format_rle must give the
    file's bytes with exactly those two newlines more, and nothing else different."""
    cells, _ = rle_ref.decode(GUN)
    assert int(cells.sum()) == 36
    want = np.zeros((128, 128), np.uint8)
    want[5:14, 5:41] = cells
    path = tmp_path / "gun.rle"
    path.write_bytes(b"#N Gosper glider gun\n" + GUN)
    with gh.Engine(128, 128, layout="bit", tblock_k=8) as e:
        assert e.load_rle(str(path), at=(5, 5)) == (36, 9)
        assert (e.download() == want).all()
        got = e.format_rle((5, 5, 9, 36))
        assert got == rle_ref.encode(cells)
        head, body = got.split(b"\n", 1)
        assert head + b"\n" == GUN[:29] and body.replace(b"\n", b"") + b"\n" == GUN_BODY and body.count(b"\n") == 3
        e.step(30)
        assert e.popcount() == 41
        e.step(30)
        assert (e.download() == g.run(want, 60, g.DEAD)).all() and e.popcount() == 46


# ------------------------------------------------------------------ the rule in the header
def life_like(board, gens, birth, survive):
    b = board.copy()
    for _ in range(gens):
        p = np.pad(b, 1)
        n = sum(np.roll(np.roll(p, dr, 0), dc, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)) - p
        n = n[1:-1, 1:-1]
        b = np.where(b == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)
    return b


def test_rule_in_the_header(gh, tmp_path):
    b = soup(12, 61, 130, 0.35)
    path = str(tmp_path / "highlife.rle")
    with gh.Engine(61, 130, layout="bit", tblock_k=3, rule="B36/S23") as e:
        e.upload(b)
        e.save_rle(path)
        text = open(path, "rb").read()
        assert text.startswith(b"x = 130, y = 61, rule = B36/S23\n") and text == rle_ref.encode(b, 0x48, 0xC)
        assert gh.rle_header(text)[:3] == (130, 61, (0x48, 0xC))
    with gh.Engine(61, 130, layout="bit", tblock_k=3) as e:
        assert e.load_rle(path, set_rule=True) == (130, 61) and e.rule == (0x48, 0xC)
        e.step(12)
        assert (e.download() == life_like(b, 12, 0x48, 0xC)).all()
    with gh.Engine(61, 130, layout="bit", tblock_k=3) as e:
        assert e.load_rle(path, set_rule=False) == (130, 61) and e.rule == rle_ref.LIFE
        e.step(12)
        assert (e.download() == life_like(b, 12, *rle_ref.LIFE)).all()


# ------------------------------------------------------------------ errors and the clock probe
def test_errors_and_clock_probe(gh):
    b = soup(2, 20, 100)
    with gh.Engine(20, 100, layout="bit") as e:
        e.upload(b)
        for text in (b"x = 5, y = 3\n3o$.o!", b"x = 5, y = 3\n6o!", b"x = 5, y = 3\n3o$2o", b"x = 5, y = 3\n3o$0o!"):
            with pytest.raises(rle_ref.RleError) as ref:
                rle_ref.decode(text)
            with pytest.raises(gh.GolError) as ex:
                e.parse_rle(text, at=(1, 1))
            assert ex.value.code == -1 and f"at byte {ref.value.offset}:" in str(ex.value)
        with pytest.raises(gh.GolError) as ex:
            e.parse_rle(b"x = 5, y = 3\n5o!", at=(18, 0))
        assert ex.value.code == -1 and "leaves the grid" in str(ex.value)
        with pytest.raises(gh.GolError) as ex:
            e.format_rle((0, 0, 21, 100))
        assert ex.value.code == -1 and "outside the grid" in str(ex.value)
        e.upload(b)
        buf, n = ctypes.create_string_buffer(16), ctypes.c_int64()
        want = rle_ref.encode(b)
        assert e.lib.gol_format_rle(e._c, 0, 0, 20, 100, buf, 16, ctypes.byref(n)) == -1 and n.value == len(want)
        e.clock_start(30000.0)
        try:
            for call in (lambda: e.rle_bytes(), lambda: e.format_rle(), lambda: e.parse_rle(b"x = 1, y = 1\no!")):
                with pytest.raises(gh.GolError) as ex:
                    call()
                assert ex.value.code == -6 and "probe" in str(ex.value)
        finally:
            e.clock_stop()
        assert e.format_rle() == want and e.generation == 0


# ------------------------------------------------------------------ bin/gol --format rle, --pattern
def _run(args, cwd, check=True):
    return subprocess.run([EXE] + args, cwd=cwd, check=check, capture_output=True, text=True, timeout=120)


def _main_name(d):
    return [f for f in os.listdir(d) if f.endswith(".gol") and "_" not in f][0][:-4]


def read_rle_part(path):
    raw = open(path, "rb").read()
    m = re.match(rb"#CXRLE Pos=(\d+),(\d+)\n", raw)
    assert m, raw[:60]
    cells, _ = rle_ref.decode(raw)
    assert raw[m.end():] == rle_ref.encode(cells)   # the part is canonical
    return (int(m.group(2)), int(m.group(1))), cells


def read_pbm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P4\n# gol (\d+) (\d+) (\d+) (\d+)\n(\d+) (\d+)\n", raw)
    assert m, raw[:60]
    ncols, nrows = int(m.group(5)), int(m.group(6))
    bits = np.frombuffer(raw[m.end():], np.uint8).reshape(nrows, (ncols + 7) // 8)
    return (int(m.group(1)), int(m.group(3))), np.unpackbits(bits, axis=1)[:, :ncols]


def test_driver_rle_snapshots_resume_and_pattern(gh, g, tmp_path):
    args = ["--mode", "dead", "--save", "--gpus", "2", "-k", "3", "--seed", "11"]
    a, t = tmp_path / "a", tmp_path / "t"
    a.mkdir()
    t.mkdir()
    _run(args + ["--format", "rle", "96", "200", "5", "20"], a)
    _run(args + ["--format", "pbm", "96", "200", "5", "20"], t)   # the twin: the same run as rasters
    name, tname = _main_name(a), _main_name(t)
    for it in (0, 5, 10, 15, 20):
        for p in range(2):
            at, cells = read_rle_part(a / f"{name}_{it}_{p}.rle")
            tat, want = read_pbm(t / f"{tname}_{it}_{p}.pbm")
            assert at == tat == (48 * p, 0) and (cells == want).all() and want.any(), (it, p)
    # resume from iteration 10: 15 and 20 come out byte for byte
    b = tmp_path / "b"
    shutil.copytree(a, b)
    for it in (15, 20):
        for p in range(2):
            (b / f"{name}_{it}_{p}.rle").unlink()
    _run(args + ["--format", "rle", "--resume", name, "--from", "10"], b)
    for it in (15, 20):
        for p in range(2):
            assert open(b / f"{name}_{it}_{p}.rle", "rb").read() == open(a / f"{name}_{it}_{p}.rle", "rb").read()
    # --pattern gun.rle@5,5 on an empty board: the oracle's board after 60 generations
    c = tmp_path / "c"
    c.mkdir()
    (c / "gun.rle").write_bytes(GUN)
    _run(["--mode", "dead", "--save", "--soup", "0", "--format", "rle", "--pattern", "gun.rle@5,5", "128", "128", "60", "60"], c)
    cname = _main_name(c)
    cells, _ = rle_ref.decode(GUN)
    start = np.zeros((128, 128), np.uint8)
    start[5:14, 5:41] = cells
    for it in (0, 60):
        at, got = read_rle_part(c / f"{cname}_{it}_0.rle")
        want = g.run(start, it, g.DEAD)
        assert at == (0, 0) and (got == want).all() and int(want.sum()) == (36, 46)[it == 60]
    # a pattern whose header names a rule sets it; --rule wins
    (c / "hl.rle").write_bytes(rle_ref.encode(soup(4, 20, 30), 0x48, 0xC))
    r = _run(["--mode", "dead", "--soup", "0", "--digest", "--pattern", "hl.rle@3,3", "64", "64", "8", "8"], c)
    r2 = _run(["--mode", "dead", "--soup", "0", "--digest", "--rule", "B36/S23", "--pattern", "hl.rle@3,3", "64", "64", "8", "8"], c)
    r3 = _run(["--mode", "dead", "--soup", "0", "--digest", "--rule", "B3/S23", "--pattern", "hl.rle@3,3", "64", "64", "8", "8"], c)
    dig = [re.findall(r"digest 8 (\w+)", x.stdout) for x in (r, r2, r3)]
    assert dig[0] and dig[0] == dig[1] and dig[0] != dig[2], dig
    r = _run(["--format", "png", "96", "200", "5", "20"], c, check=False)
    assert r.returncode == 1 and "--format must be" in r.stdout
