"""ctypes binding of ``libgolhip.so`` (the C ABI declared in ``include/golhip.h``).

Host-side mirror of the reference's hot-path interface.  The reference is a
C++ program whose generation loop (main.cpp:291-305) calls

    updateBoard(board, board2, options)      main.cpp:93-103  -> Engine.update_board / step
    swap(board, board2)                      main.cpp:294-296 -> ping-pong inside the context
    distr_borders(board, nbr, comm, options) main.cpp:36-65   -> halo exchange inside step
    initializeBoard(board, options, rank)    main.cpp:68-77   -> Engine.initialize_board

This module never computes a generation itself: every call goes to the HIP
library, and importing it on a machine without ``libgolhip.so`` raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

LAYOUT = {"byte": 0, "bit": 1}
BOUNDARY = {"dead": 0, "serial_compat": 1, "mesh_compat": 2, "torus": 3}
INIT = {"stream": 0, "serial": 1, "mesh": 2}
COPY_OPS = {"replace": 0, "or": 1, "xor": 2}   # GOL_COPY_*
SERIAL_SEED = 1804289383

OPT_CHUNK_ROWS = 1
OPT_KERNEL_TIMING = 2
OPT_OVERLAP = 4
OPT_BYTE_CORE = 5
OPT_TEXT_BLOCK_BYTES = 10
OPT_SCHEDULE_TRIAL = 11
OPT_INTERIOR_SPLIT = 12
OPT_SCHED_TRACE = 13
OPT_COMM_TIMING = 14
OPT_HALO_EXCHANGE = 15
OPT_RULE_KERNEL = 16
OPT_RULE_COMPILED = 17
RULE_PATHS = ("tuned", "generic", "compiled")   # GOL_RULE_PATH_*
# retired in 0.2 (accepted by gol_set_option as no-ops; kept so old callers still run)
OPT_WORDS_PER_LANE = 3
OPT_SPLIT = 6

ERRORS = {0: "OK", -1: "EINVAL", -2: "EHIP", -3: "ERCCL", -4: "ENOMEM", -5: "EUNSUPPORTED", -6: "ESTATE"}

EXPORTS = [
    "gol_create", "gol_create_rank", "gol_get_unique_id", "gol_slab_plan", "gol_set_option", "gol_get_option",
    "gol_init_glibc", "gol_upload", "gol_upload_window", "gol_step", "gol_sync", "gol_download",
    "gol_download_window", "gol_popcount", "gol_generation", "gol_kernel_time", "gol_last_error",
    "gol_destroy", "gol_version", "gol_text_bytes", "gol_format_text", "gol_write_text", "gol_parse_text",
    "gol_read_text", "gol_download_window_async", "gol_clock_start", "gol_clock_stop", "gol_rccl_selftest",
    "gol_sched_trace", "gol_comm_time", "gol_parse_rule", "gol_set_rule", "gol_get_rule",
    "gol_digest", "gol_digest_window", "gol_digest_async",
    "gol_density_dims", "gol_density", "gol_density_window", "gol_density_async",
    "gol_bits_row_bytes", "gol_download_bits", "gol_download_bits_window", "gol_download_bits_window_async",
    "gol_upload_bits", "gol_upload_bits_window",
    "gol_fill_threshold", "gol_fill_random", "gol_fill_random_window",
    "gol_copy_window", "gol_copy",
    "gol_compiled_rule", "gol_rule_path",
    "gol_rle_header", "gol_rle_bytes", "gol_format_rle", "gol_write_rle", "gol_parse_rle", "gol_read_rle",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOL_LIB") or os.path.join(_HERE, "libgolhip.so")
_lib = None


class GolError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


def load() -> ctypes.CDLL:
    """Load libgolhip.so; raise if it was not built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C mpi_amd` or __graft_entry__.build()"
        )
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    i64, i32, u32 = ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
    u8p = ctypes.POINTER(ctypes.c_uint8)
    i64p = ctypes.POINTER(ctypes.c_int64)
    dp = ctypes.POINTER(ctypes.c_double)
    sig = {
        "gol_create": ([ctypes.POINTER(P), i64, i64, i32, i32, i32, i32, i32], i32),
        "gol_create_rank": ([ctypes.POINTER(P), i64, i64, i32, i32, i32, u8p, i32, i32, i32, i32], i32),
        "gol_get_unique_id": ([u8p], i32),
        "gol_slab_plan": ([i64, i32, i32, i64p, i64p], i32),
        "gol_set_option": ([P, i32, i64], i32),
        "gol_get_option": ([P, i32, i64p], i32),
        "gol_init_glibc": ([P, i32, u32], i32),
        "gol_upload": ([P, u8p, i64], i32),
        "gol_upload_window": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_step": ([P, i64], i32),
        "gol_sync": ([P, dp], i32),
        "gol_download": ([P, u8p, i64], i32),
        "gol_download_window": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_popcount": ([P, i64p], i32),
        "gol_generation": ([P, i64p], i32),
        "gol_kernel_time": ([P, dp, i64p, i32], i32),
        "gol_comm_time": ([P, dp, dp, i64p, i32], i32),
        "gol_sched_trace": ([P, i64p, i64, i64p], i32),
        "gol_last_error": ([P], ctypes.c_char_p),
        "gol_destroy": ([P], None),
        "gol_version": ([], ctypes.c_char_p),
        "gol_text_bytes": ([i64, i64], i64),
        "gol_format_text": ([P, i64, i64, i64, i64, ctypes.c_char_p, i64], i32),
        "gol_write_text": ([P, i64, i64, i64, i64, i32], i32),
        "gol_parse_text": ([P, i64, i64, i64, i64, ctypes.c_char_p, i64], i32),
        "gol_read_text": ([P, i64, i64, i64, i64, i32], i32),
        "gol_download_window_async": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_clock_start": ([P, ctypes.c_double], i32),
        "gol_clock_stop": ([P, dp, dp], i32),
        "gol_rccl_selftest": ([i32, i64, i32, dp, ctypes.c_char_p, i32], i32),
        "gol_parse_rule": ([ctypes.c_char_p, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
        "gol_set_rule": ([P, u32, u32], i32),
        "gol_get_rule": ([P, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
        "gol_digest": ([P, ctypes.POINTER(ctypes.c_uint64)], i32),
        "gol_digest_window": ([P, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_uint64)], i32),
        "gol_digest_async": ([P, ctypes.POINTER(ctypes.c_uint64)], i32),
        "gol_density_dims": ([i64, i64, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)], i32),
        "gol_density": ([P, i64, i64, ctypes.POINTER(u32), i64], i32),
        "gol_density_window": ([P, i64, i64, i64, i64, i64, i64, ctypes.POINTER(u32), i64], i32),
        "gol_density_async": ([P, i64, i64, ctypes.POINTER(u32), i64], i32),
        "gol_bits_row_bytes": ([i64], i64),
        "gol_download_bits": ([P, u8p, i64], i32),
        "gol_download_bits_window": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_download_bits_window_async": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_upload_bits": ([P, u8p, i64], i32),
        "gol_upload_bits_window": ([P, i64, i64, i64, i64, u8p, i64], i32),
        "gol_fill_threshold": ([ctypes.c_double, ctypes.POINTER(ctypes.c_uint64)], i32),
        "gol_fill_random": ([P, ctypes.c_uint64, ctypes.c_uint64], i32),
        "gol_fill_random_window": ([P, i64, i64, i64, i64, ctypes.c_uint64, ctypes.c_uint64], i32),
        "gol_copy_window": ([P, i64, i64, P, i64, i64, i64, i64, i32], i32),
        "gol_copy": ([P, P], i32),
        "gol_compiled_rule": ([i32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_char_p)], i32),
        "gol_rule_path": ([P, ctypes.POINTER(i32)], i32),
        "gol_rle_header": ([ctypes.c_char_p, i64, i64p, i64p, ctypes.POINTER(u32), ctypes.POINTER(u32),
                            ctypes.POINTER(i32), i64p], i32),
        "gol_rle_bytes": ([P, i64, i64, i64, i64, i64p], i32),
        "gol_format_rle": ([P, i64, i64, i64, i64, ctypes.c_char_p, i64, i64p], i32),
        "gol_write_rle": ([P, i64, i64, i64, i64, i32], i32),
        "gol_parse_rle": ([P, i64, i64, ctypes.c_char_p, i64, i64p, i64p], i32),
        "gol_read_rle": ([P, i64, i64, i32, i64p, i64p], i32),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def version() -> str:
    return load().gol_version().decode()


def slab_plan(rows: int, world: int, rank: int) -> tuple[int, int]:
    """Row range (row0, nrows) of slab `rank` of `world` (host-only, no GPU)."""
    r0, n = ctypes.c_int64(), ctypes.c_int64()
    rc = load().gol_slab_plan(rows, world, rank, ctypes.byref(r0), ctypes.byref(n))
    if rc:
        raise GolError(rc, "gol_slab_plan")
    return r0.value, n.value


def parse_rule(text: str) -> tuple[int, int]:
    """(birth, survive) masks of a life-like rule: "B36/S23", "S23/B36" (either letter
    case) or the legacy survive/birth form "23/3".  Bit n = n live neighbours.  Host-only."""
    b, s = ctypes.c_uint32(), ctypes.c_uint32()
    rc = load().gol_parse_rule(text.encode(), ctypes.byref(b), ctypes.byref(s))
    if rc:
        raise GolError(rc, f"gol_parse_rule: not a B/S rule: {text!r}")
    return b.value, s.value


def rle_header(text: bytes | str) -> tuple[int, int, tuple[int, int] | None, int]:
    """(x, y, rule, body) of an RLE text's header line (behind any '#' lines): the pattern's box,
    the (birth, survive) masks of its `rule = ...` or None if it names none, and the offset of the
    first body byte (gol_rle_header).  Host-only."""
    t = text.encode() if isinstance(text, str) else bytes(text)
    x, y, body = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    b, s, has = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    rc = load().gol_rle_header(t, len(t), ctypes.byref(x), ctypes.byref(y), ctypes.byref(b), ctypes.byref(s),
                               ctypes.byref(has), ctypes.byref(body))
    if rc:
        raise GolError(rc, "gol_rle_header: not an RLE header")
    return x.value, y.value, ((b.value, s.value) if has.value else None), body.value


def compiled_rules() -> list[tuple[str, int, int]]:
    """(name, birth, survive) of every rule with a kernel compiled for it, in list order
    (gol_compiled_rule).  Host-only."""
    out = []
    while True:
        b, s, name = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_char_p()
        if load().gol_compiled_rule(len(out), ctypes.byref(b), ctypes.byref(s), ctypes.byref(name)):
            return out
        out.append((name.value.decode(), b.value, s.value))


def density_dims(nrows: int, ncols: int, tile_rows: int, tile_cols: int) -> tuple[int, int]:
    """(trows, tcols) of the density map of a nrows × ncols window: ceil(nrows / tile_rows),
    ceil(ncols / tile_cols).  Host-only."""
    tr, tc = ctypes.c_int64(), ctypes.c_int64()
    rc = load().gol_density_dims(nrows, ncols, tile_rows, tile_cols, ctypes.byref(tr), ctypes.byref(tc))
    if rc:
        raise GolError(rc, "gol_density_dims: sizes >= 0 and tiles >= 1")
    return tr.value, tc.value


def bits_row_bytes(ncols: int) -> int:
    """Bytes of one packed row of ncols cells: ceil(ncols / 8).  Host-only."""
    n = load().gol_bits_row_bytes(ncols)
    if n < 0:
        raise GolError(n, "gol_bits_row_bytes: ncols >= 0")
    return n


def fill_threshold(p: float) -> int:
    """The threshold of density p for Engine.fill_random: round(p * 2^32), 0 <= p <= 1.  Host-only."""
    t = ctypes.c_uint64()
    rc = load().gol_fill_threshold(p, ctypes.byref(t))
    if rc:
        raise GolError(rc, f"gol_fill_threshold: a density in [0, 1], not {p!r}")
    return t.value


def unique_id() -> bytes:
    """RCCL bootstrap blob (rank 0 creates it, the caller broadcasts it)."""
    buf = (ctypes.c_uint8 * 128)()
    rc = load().gol_get_unique_id(buf)
    if rc:
        raise GolError(rc, "gol_get_unique_id (RCCL unavailable?)")
    return bytes(buf)


def rccl_selftest(device: int = 0, nbytes: int = 8 * 16896, reps: int = 20) -> tuple[float, str]:
    """Real RCCL through the library's own binding: a 1-rank communicator sends
    two halo-sized messages to itself per group, `reps` groups; raises on any
    error or byte mismatch.  Returns (device µs per group, message)."""
    us = ctypes.c_double()
    msg = ctypes.create_string_buffer(512)
    rc = load().gol_rccl_selftest(device, nbytes, reps, ctypes.byref(us), msg, len(msg))
    if rc:
        raise GolError(rc, msg.value.decode())
    return us.value, msg.value.decode()


def part_geometry(path: str) -> tuple[int, int, int, int, int]:
    """(row0, col0, nrows, ncols, body_offset) of a `.gol` part file: origin from
    the two header lines, shape from the body (main.cpp:106-129 layout)."""
    with open(path, "rb") as f:
        l1, l2 = f.readline(), f.readline()
        off = f.tell()
        first = f.readline()
        size = os.fstat(f.fileno()).st_size
    row0, col0 = int(l1.split()[0]), int(l2.split()[0])
    if not first.endswith(b"\n") or len(first) % 2 == 0:
        raise GolError(-1, f"{path}: malformed first body row")
    rowlen = len(first)
    if (size - off) % rowlen:
        raise GolError(-1, f"{path}: body of {size - off} bytes is not a whole number of {rowlen}-byte rows")
    return row0, col0, (size - off) // rowlen, (rowlen - 1) // 2, off


def _u8(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u32(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class Engine:
    """One Game-of-Life board on the GPU(s).

    Single process: ``Engine(rows, cols, n_gpus=N)`` cuts the grid into N row
    slabs (slab s on device s % visible).  One process per GPU:
    ``Engine(rows, cols, rank=r, world=W, device=d, uid=blob)``.
    """

    def __init__(self, rows: int, cols: int, *, n_gpus: int = 1, layout: str = "bit",
                 boundary: str = "dead", mesh_m: int = 1, tblock_k: int = 1,
                 rank: int | None = None, world: int | None = None, device: int = 0,
                 uid: bytes | None = None, rule: str | tuple[int, int] | None = None):
        self.lib = load()
        self._pending = []   # arrays the library fills at the next synchronising call
        self.rows, self.cols = rows, cols
        self.layout, self.boundary, self.tblock_k = layout, boundary, tblock_k
        self.mesh_m, self.n_gpus = mesh_m, n_gpus
        self._rank_ctx = rank is not None
        self._c = ctypes.c_void_p()
        if rank is None:
            rc = self.lib.gol_create(ctypes.byref(self._c), rows, cols, n_gpus, LAYOUT[layout],
                                     BOUNDARY[boundary], mesh_m, tblock_k)
            self.rank, self.world = 0, 1
        else:
            u = None
            if uid is not None:
                u = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
            rc = self.lib.gol_create_rank(ctypes.byref(self._c), rows, cols, rank, world, device, u,
                                          LAYOUT[layout], BOUNDARY[boundary], mesh_m, tblock_k)
            self.rank, self.world = rank, world
        if rc:
            raise GolError(rc, "gol_create failed (see stderr)")
        if rule is not None:
            try:
                self.set_rule(rule)
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------ plumbing
    def _chk(self, rc: int, what: str):
        if rc:
            raise GolError(rc, f"{what}: {self.lib.gol_last_error(self._c).decode()}")

    def close(self):
        if self._c:
            self.lib.gol_destroy(self._c)
            self._c = ctypes.c_void_p()
        self._pending = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int):
        self._chk(self.lib.gol_set_option(self._c, opt, value), "gol_set_option")

    def get_option(self, opt: int) -> int:
        v = ctypes.c_int64()
        self._chk(self.lib.gol_get_option(self._c, opt, ctypes.byref(v)), "gol_get_option")
        return v.value

    def set_rule(self, rule: str | tuple[int, int]):
        """Life-like rule from the next step on: B/S text (parse_rule) or (birth, survive)
        masks.  Synchronises.  Rules other than B3/S23: bit layout, tblock_k 1..7, dead or
        torus boundary.  RCCL mode: collective (set it alike on every rank)."""
        birth, survive = parse_rule(rule) if isinstance(rule, str) else rule
        self._chk(self.lib.gol_set_rule(self._c, birth, survive), "gol_set_rule")

    @property
    def rule(self) -> tuple[int, int]:
        """(birth, survive) masks of the rule in force."""
        b, s = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.lib.gol_get_rule(self._c, ctypes.byref(b), ctypes.byref(s)), "gol_get_rule")
        return b.value, s.value

    @property
    def rule_path(self) -> str:
        """What the next step launches for the rule in force: "tuned" (B3/S23), "compiled"
        (a rule of compiled_rules(), OPT_RULE_COMPILED) or "generic" (gol_rule_path)."""
        p = ctypes.c_int()
        self._chk(self.lib.gol_rule_path(self._c, ctypes.byref(p)), "gol_rule_path")
        return RULE_PATHS[p.value]

    # ------------------------------------------------------------ board state
    def initialize_board(self, mode: str = "stream", seed: int = 1):
        """initializeBoard (main.cpp:68-77 / main_serial.cpp:34-43), on device."""
        self._chk(self.lib.gol_init_glibc(self._c, INIT[mode], seed), "gol_init_glibc")

    def upload(self, board: np.ndarray):
        b = np.ascontiguousarray(board != 0, dtype=np.uint8)   # bool cells (main.cpp:73)
        assert b.shape == (self.rows, self.cols)
        self._chk(self.lib.gol_upload(self._c, _u8(b), b.shape[1]), "gol_upload")

    def upload_window(self, row0: int, col0: int, win: np.ndarray):
        w = np.ascontiguousarray(win != 0, dtype=np.uint8)
        self._chk(self.lib.gol_upload_window(self._c, row0, col0, w.shape[0], w.shape[1], _u8(w),
                                             w.shape[1]), "gol_upload_window")

    def download(self) -> np.ndarray:
        out = np.zeros((self.rows, self.cols), np.uint8)
        self._chk(self.lib.gol_download(self._c, _u8(out), self.cols), "gol_download")
        return out

    def download_window(self, row0: int, col0: int, nrows: int, ncols: int) -> np.ndarray:
        out = np.zeros((nrows, ncols), np.uint8)
        self._chk(self.lib.gol_download_window(self._c, row0, col0, nrows, ncols, _u8(out), ncols),
                  "gol_download_window")
        return out

    def download_window_async(self, row0: int, col0: int, nrows: int, ncols: int) -> np.ndarray:
        """Enqueue a copy of the window behind the steps enqueued so far; the
        returned array is filled by the next synchronising call (sync, popcount,
        download...).  Keep it alive until then."""
        out = np.zeros((nrows, ncols), np.uint8)
        self._chk(self.lib.gol_download_window_async(self._c, row0, col0, nrows, ncols, _u8(out), ncols),
                  "gol_download_window_async")
        self._pending.append(out)   # kept alive here until a synchronising call has filled it
        return out

    # ------------------------------------------------------------ packed bits
    # Rows of ceil(ncols / 8) bytes, MSB first: np.packbits(window, axis=1), a PBM P4 raster.
    def download_bits(self) -> np.ndarray:
        """The board as packed rows, packed on the device: np.packbits(download(), axis=1)
        at an eighth of the transfer.  Rank contexts fill their slab's rows only."""
        out = np.zeros((self.rows, bits_row_bytes(self.cols)), np.uint8)
        self._chk(self.lib.gol_download_bits(self._c, _u8(out), out.shape[1]), "gol_download_bits")
        return out

    def download_bits_window(self, row0: int, col0: int, nrows: int, ncols: int) -> np.ndarray:
        out = np.zeros((nrows, bits_row_bytes(ncols)), np.uint8)
        self._chk(self.lib.gol_download_bits_window(self._c, row0, col0, nrows, ncols, _u8(out), out.shape[1]),
                  "gol_download_bits_window")
        return out

    def download_bits_window_async(self, row0: int, col0: int, nrows: int, ncols: int) -> np.ndarray:
        """download_window_async with packed rows: filled by the next synchronising call."""
        out = np.zeros((nrows, bits_row_bytes(ncols)), np.uint8)
        self._chk(self.lib.gol_download_bits_window_async(self._c, row0, col0, nrows, ncols, _u8(out), out.shape[1]),
                  "gol_download_bits_window_async")
        self._pending.append(out)   # kept alive here until a synchronising call has filled it
        return out

    def upload_bits(self, arr: np.ndarray):
        """Packed rows (uint8, shape (rows, ceil(cols / 8))) -> the board; pad bits are ignored."""
        a = np.ascontiguousarray(arr, dtype=np.uint8)
        assert a.shape == (self.rows, bits_row_bytes(self.cols)), a.shape
        self._chk(self.lib.gol_upload_bits(self._c, _u8(a), a.shape[1]), "gol_upload_bits")

    def upload_bits_window(self, row0: int, col0: int, ncols: int, arr: np.ndarray):
        """Packed rows of an arr.shape[0] × ncols window (the array's width is in bytes)."""
        a = np.ascontiguousarray(arr, dtype=np.uint8)
        assert a.ndim == 2 and a.shape[1] == bits_row_bytes(ncols), a.shape
        self._chk(self.lib.gol_upload_bits_window(self._c, row0, col0, a.shape[0], ncols, _u8(a), a.shape[1]),
                  "gol_upload_bits_window")

    # ------------------------------------------------------------ random fill
    def fill_random(self, density: float = 0.5, seed: int = 0, window: tuple[int, int, int, int] | None = None,
                    threshold: int | None = None):
        """A seeded soup written on the device: cell (r, c) is live iff X(seed, r, c) < threshold
        (include/golhip.h, tests/fill_ref.py), threshold = fill_threshold(density) unless given
        (0 .. 2^32).  window = (row0, col0, nrows, ncols): only those cells change, and they equal
        the same cells of a whole-board fill.  The generation and the rule stay as they are.
        Rank contexts write the rows they hold.  Synchronises."""
        t = fill_threshold(density) if threshold is None else threshold
        if window is None:
            self._chk(self.lib.gol_fill_random(self._c, seed, t), "gol_fill_random")
        else:
            self._chk(self.lib.gol_fill_random_window(self._c, *window, seed, t), "gol_fill_random_window")
        self._pending = []

    # ------------------------------------------------------------ board-to-board copy
    def copy_from(self, src: "Engine", window: tuple[int, int, int, int] | None = None,
                  at: tuple[int, int] = (0, 0), op: str = "replace"):
        """Cells of `src` merged into this board on the device (gol_copy_window): window =
        (row0, col0, nrows, ncols) of src (default its whole board) lands with its corner at
        `at`; op = "replace", "or" or "xor".  The two engines may differ in layout, tblock_k,
        boundary, slab count and size; the generation and rule of both stay as they are.
        src may be this engine when the two rectangles are disjoint.  Rank contexts write
        the rows they hold, whose source rows src must hold.  Synchronises both engines."""
        if op not in COPY_OPS:
            raise ValueError(f"copy_from: op must be one of {sorted(COPY_OPS)}")
        row0, col0, nrows, ncols = (0, 0, src.rows, src.cols) if window is None else window
        self._chk(self.lib.gol_copy_window(self._c, at[0], at[1], src._c, row0, col0, nrows, ncols, COPY_OPS[op]),
                  "gol_copy_window")
        self._pending = []
        src._pending = []

    def clone(self, **overrides) -> "Engine":
        """A new single-process Engine of the same rows, cols, boundary, mesh_m, layout,
        tblock_k, n_gpus and rule — except where overridden — with this board copied in on
        the device.  Its generation starts at 0.  GolError where the target cannot run the
        rule (set_rule's limits).  A rank context cannot be cloned this way (ValueError)."""
        if self._rank_ctx:
            raise ValueError("clone: a rank context holds one slab of the board; create the target ranks and copy_from")
        kw = dict(n_gpus=self.n_gpus, layout=self.layout, boundary=self.boundary, mesh_m=self.mesh_m,
                  tblock_k=self.tblock_k, rule=self.rule)
        rows, cols = overrides.pop("rows", self.rows), overrides.pop("cols", self.cols)
        kw.update(overrides)
        e = Engine(rows, cols, **kw)
        try:
            e.copy_from(self, (0, 0, min(rows, self.rows), min(cols, self.cols)))
        except Exception:
            e.close()
            raise
        return e

    def period(self, limit: int, batch: int = 64):
        """The smallest p in 1 .. limit at which the board returns to its present state, or
        None: the exact period that find_repeat cannot give.  A clone of the board is
        stepped one generation at a time with a digest_async after each, one sync per
        `batch` generations, and compared against this board's digest; this engine does
        not move.  (Equal digests: equal boards up to the digest's collision odds.)"""
        if limit < 1 or batch < 1 or batch > 1024:
            raise ValueError("period: limit >= 1 and 1 <= batch <= 1024")
        want = self.digest()
        with self.clone() as e:
            p = 0
            while p < limit:
                outs = []
                for _ in range(min(batch, limit - p)):
                    e.step(1)
                    p += 1
                    outs.append((p, e.digest_async()))
                e.sync()
                for g, o in outs:
                    if (int(o[0]), int(o[1])) == want:
                        return g
        return None

    # ------------------------------------------------------------ digest
    def digest(self) -> tuple[int, int]:
        """128-bit digest of the logical board (two 64-bit lanes), computed on the device:
        equal for every layout, tblock_k, boundary storage, slab count and transport, and
        equal to the digest of download() (tests/digest_ref.py).  Rank contexts return
        their slab's part; the parts add mod 2^64.  Synchronises."""
        d = (ctypes.c_uint64 * 2)()
        self._chk(self.lib.gol_digest(self._c, d), "gol_digest")
        self._pending = []
        return int(d[0]), int(d[1])

    def digest_window(self, row0: int, col0: int, nrows: int, ncols: int) -> tuple[int, int]:
        """Digest of a window (global coordinates; digests of disjoint windows add mod
        2^64).  Rows this context does not hold contribute nothing.  Synchronises."""
        d = (ctypes.c_uint64 * 2)()
        self._chk(self.lib.gol_digest_window(self._c, row0, col0, nrows, ncols, d), "gol_digest_window")
        self._pending = []
        return int(d[0]), int(d[1])

    def digest_async(self) -> np.ndarray:
        """Enqueue a whole-board digest behind the steps enqueued so far; the returned
        array of 2 uint64 is filled by the next synchronising call.  At most 1024 pending
        (GolError ESTATE beyond: sync first)."""
        out = np.zeros(2, np.uint64)
        self._chk(self.lib.gol_digest_async(self._c, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
                  "gol_digest_async")
        self._pending.append(out)   # kept alive here until a synchronising call has filled it
        return out

    def find_repeat(self, max_generations: int, every: int | None = None, batch: int = 64):
        """Step until the board's digest repeats: `every` generations at a time (default
        tblock_k), a digest_async after each, one sync per `batch` checks — the engine
        never drains between checks; the comparison is host-side bookkeeping.  Returns
        (generation_first_seen, generation_repeated) for the first digest seen before
        (the digest of the current generation is included), or None once max_generations
        more generations have been stepped (whole multiples of `every`).
        The distance is a multiple of `every`, and the board's true period divides it
        (`period` finds the exact one);
        generation_first_seen is the first CHECKED generation inside the cycle.  The
        engine is left at the end of the batch in which the repeat was found (see
        `generation`), not at generation_repeated.  A rank context compares its own slab
        only: a board-wide conclusion needs every rank's answer (or the summed parts)."""
        every = self.tblock_k if every is None else every
        if every < 1 or batch < 1 or batch > 1024:
            raise ValueError("find_repeat: every >= 1 and 1 <= batch <= 1024")
        seen = {self.digest(): self.generation}
        gen, left = self.generation, max_generations // every
        while left > 0:
            outs = []
            for _ in range(min(batch, left)):
                self.step(every)
                gen += every
                outs.append((gen, self.digest_async()))
            left -= len(outs)
            self.sync()
            for g, o in outs:
                key = (int(o[0]), int(o[1]))
                if key in seen:
                    return seen[key], g
                seen[key] = g
        return None

    # ------------------------------------------------------------ density
    def density(self, tile_rows: int, tile_cols: int | None = None) -> np.ndarray:
        """Live cells per tile of tile_rows × tile_cols cells (tile_cols: a multiple of 32,
        default tile_rows), computed on the device: a uint32 array of shape
        density_dims(rows, cols, ...), equal to the map of download()
        (tests/density_ref.py); edge tiles are clipped to the board.  Rank contexts return
        the counts of their own rows (0 elsewhere); the maps add.  Synchronises."""
        return self.density_window(0, 0, self.rows, self.cols, tile_rows, tile_cols)

    def density_window(self, row0: int, col0: int, nrows: int, ncols: int, tile_rows: int,
                       tile_cols: int | None = None) -> np.ndarray:
        """Density map of a window (global coordinates, col0 a multiple of 32), tiles
        counted from its origin.  Synchronises."""
        tile_cols = tile_rows if tile_cols is None else tile_cols
        out = np.zeros(density_dims(nrows, ncols, tile_rows, tile_cols), np.uint32)
        ld = max(1, out.shape[1])
        self._chk(self.lib.gol_density_window(self._c, row0, col0, nrows, ncols, tile_rows, tile_cols, _u32(out), ld),
                  "gol_density_window")
        self._pending = []
        return out

    def density_async(self, tile_rows: int, tile_cols: int | None = None) -> np.ndarray:
        """Enqueue a whole-board density map behind the steps enqueued so far; the
        returned uint32 array is filled by the next synchronising call."""
        tile_cols = tile_rows if tile_cols is None else tile_cols
        out = np.zeros(density_dims(self.rows, self.cols, tile_rows, tile_cols), np.uint32)
        self._chk(self.lib.gol_density_async(self._c, tile_rows, tile_cols, _u32(out), max(1, out.shape[1])),
                  "gol_density_async")
        self._pending.append(out)   # kept alive here until a synchronising call has filled it
        return out

    def clock_start(self, max_ms: float):
        """Start the clock probe (one wave on its own stream, stops by itself after max_ms)."""
        self._chk(self.lib.gol_clock_start(self._c, max_ms), "gol_clock_start")

    def clock_stop(self) -> tuple[float, float]:
        """(shader clock in MHz, span in ms) over the probe's lifetime."""
        mhz, span = ctypes.c_double(), ctypes.c_double()
        self._chk(self.lib.gol_clock_stop(self._c, ctypes.byref(mhz), ctypes.byref(span)), "gol_clock_stop")
        return mhz.value, span.value

    # ------------------------------------------------------------ snapshot text
    def format_text(self, row0: int, col0: int, nrows: int, ncols: int) -> bytes:
        """`.gol` part-file body of a window (main.cpp:106-129), formatted on the device."""
        n = self.lib.gol_text_bytes(nrows, ncols)
        buf = ctypes.create_string_buffer(max(n, 1))
        self._chk(self.lib.gol_format_text(self._c, row0, col0, nrows, ncols, buf, n), "gol_format_text")
        return buf.raw[:n]

    def parse_text(self, row0: int, col0: int, nrows: int, ncols: int, text: bytes):
        """Inverse of format_text: load a window from `.gol` body text (snapshot resume)."""
        self._chk(self.lib.gol_parse_text(self._c, row0, col0, nrows, ncols, text, len(text)), "gol_parse_text")

    def save_part(self, path: str, row0: int, nrows: int, *, col0: int = 0, ncols: int | None = None,
                  header: tuple[int, int, int, int] | None = None):
        """Write one part file: the two header lines (default: inclusive ranges,
        main.cpp:255-258) and the device-formatted body, streamed to the fd."""
        ncols = self.cols - col0 if ncols is None else ncols
        h = header or (row0, row0 + nrows - 1, col0, col0 + ncols - 1)
        with open(path, "wb") as f:
            f.write(f"{h[0]} {h[1]}\n{h[2]} {h[3]}\n".encode())
            f.flush()
            self._chk(self.lib.gol_write_text(self._c, row0, col0, nrows, ncols, f.fileno()), "gol_write_text")

    def load_part(self, path: str) -> tuple[int, int, int, int]:
        """Read one part file back (either header convention): the window's
        origin is the header's first row / column, its shape comes from the
        body (row length and byte count).  Returns (row0, col0, nrows, ncols)."""
        row0, col0, nrows, ncols, off = part_geometry(path)
        fd = os.open(path, os.O_RDONLY)
        try:
            os.lseek(fd, off, os.SEEK_SET)
            self._chk(self.lib.gol_read_text(self._c, row0, col0, nrows, ncols, fd), "gol_read_text")
        finally:
            os.close(fd)
        return row0, col0, nrows, ncols

    # ------------------------------------------------------------ RLE pattern text
    def _rle_window(self, window):
        return (0, 0, self.rows, self.cols) if window is None else tuple(int(v) for v in window)

    def rle_bytes(self, window=None) -> int:
        """Bytes of format_rle(window), header included: the two counting passes on the device."""
        n = ctypes.c_int64()
        self._chk(self.lib.gol_rle_bytes(self._c, *self._rle_window(window), ctypes.byref(n)), "gol_rle_bytes")
        return n.value

    def format_rle(self, window=None) -> bytes:
        """The RLE text (header with the rule in force, canonical body) of window = (row0, col0,
        nrows, ncols), default the whole board, encoded on the device."""
        w = self._rle_window(window)
        cap = self.rle_bytes(w)
        buf = ctypes.create_string_buffer(max(cap, 1))
        n = ctypes.c_int64()
        self._chk(self.lib.gol_format_rle(self._c, *w, buf, cap, ctypes.byref(n)), "gol_format_rle")
        return buf.raw[:n.value]

    def save_rle(self, path: str, window=None):
        """format_rle streamed to a file."""
        with open(path, "wb") as f:
            self._chk(self.lib.gol_write_rle(self._c, *self._rle_window(window), f.fileno()), "gol_write_rle")

    def parse_rle(self, text: bytes | str, at: tuple[int, int] = (0, 0)) -> tuple[int, int]:
        """Load an RLE text: its x × y box at `at` = (row, col) is replaced.  Returns (x, y).
        The header's rule is not applied (rle_header + set_rule, or load_rle(set_rule=True))."""
        t = text.encode() if isinstance(text, str) else bytes(text)
        x, y = ctypes.c_int64(), ctypes.c_int64()
        self._chk(self.lib.gol_parse_rle(self._c, at[0], at[1], t, len(t), ctypes.byref(x), ctypes.byref(y)),
                  "gol_parse_rle")
        return x.value, y.value

    def load_rle(self, path: str, at: tuple[int, int] = (0, 0), set_rule: bool = False) -> tuple[int, int]:
        """parse_rle from a file, read in chunks.  set_rule: apply the header's rule (if it names
        one) before anything is written."""
        if set_rule:
            with open(path, "rb") as f:
                head = f.read(1 << 16)
            rule = rle_header(head)[2]
            if rule is not None:
                self.set_rule(rule)
        x, y = ctypes.c_int64(), ctypes.c_int64()
        fd = os.open(path, os.O_RDONLY)
        try:
            self._chk(self.lib.gol_read_rle(self._c, at[0], at[1], fd, ctypes.byref(x), ctypes.byref(y)),
                      "gol_read_rle")
        finally:
            os.close(fd)
        return x.value, y.value

    # ------------------------------------------------------------ hot path
    def step(self, generations: int = 1):
        """updateBoard + swap + distr_borders, `generations` times (async)."""
        self._chk(self.lib.gol_step(self._c, generations), "gol_step")

    update_board = step

    def sync(self) -> float:
        ms = ctypes.c_double()
        self._chk(self.lib.gol_sync(self._c, ctypes.byref(ms)), "gol_sync")
        self._pending = []
        return ms.value

    def popcount(self) -> int:
        v = ctypes.c_int64()
        self._chk(self.lib.gol_popcount(self._c, ctypes.byref(v)), "gol_popcount")
        self._pending = []
        return v.value

    @property
    def generation(self) -> int:
        v = ctypes.c_int64()
        self._chk(self.lib.gol_generation(self._c, ctypes.byref(v)), "gol_generation")
        return v.value

    def sched_trace(self):
        """The recorded schedule (GOL_OPT_SCHED_TRACE) as an (n, 7) int64 array
        (kind, stream, event, slab, buffer, row0, row1); clears the record."""
        n = ctypes.c_int64()
        self._chk(self.lib.gol_sched_trace(self._c, None, 0, ctypes.byref(n)), "gol_sched_trace")
        out = np.zeros((n.value, 7), np.int64)
        self._chk(self.lib.gol_sched_trace(self._c, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n.value,
                                           ctypes.byref(n)), "gol_sched_trace")
        return out

    def comm_time(self, reset: bool = False) -> tuple[float, float, int]:
        """(exchange ms, bands ms, k-steps) of the comm stream (GOL_OPT_COMM_TIMING)."""
        ex, bd, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self._chk(self.lib.gol_comm_time(self._c, ctypes.byref(ex), ctypes.byref(bd), ctypes.byref(n), int(reset)),
                  "gol_comm_time")
        self._pending = []
        return ex.value, bd.value, n.value

    def kernel_time(self, reset: bool = False) -> tuple[float, int]:
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._chk(self.lib.gol_kernel_time(self._c, ctypes.byref(ms), ctypes.byref(n), int(reset)),
                  "gol_kernel_time")
        self._pending = []
        return ms.value, n.value
