/*
 * golhip.h — C ABI of the MI355X-native Game-of-Life engine (libgolhip.so).
 *
 * The reference (arthurdecloedt/mpi) has no plugin or FFI API; its hot path is
 * two C++ free functions called from the generation loop of main():
 *
 *   void updateBoard(bool **board, bool **nboard, distrOpt options);            main.cpp:93-103
 *   void distr_borders(bool **board, neighbours nbr, MPI_Comm, distrOpt &);     main.cpp:36-65
 *   void updateBoard(bool **board, distrOpt options);            main_serial.cpp:45-71
 *   void initializeBoard(bool **board, distrOpt options[, int rank]);
 *                                        main.cpp:68-77, main_serial.cpp:34-43
 *
 * plus the MPI runtime around them (MPI_Init/Cart_create/Bcast/Barrier/Reduce,
 * main.cpp:154-164, 233-254, 280-324).  This header is the seam that replaces
 * all of it: one opaque context owns the device boards (ping-pong buffers per
 * row slab), the HIP streams and, for one-process-per-GPU runs, an RCCL
 * communicator for the halo rows.  Plain C types only; no torch, no C++.
 *
 * Conventions
 *  - Every function returns GOL_OK (0) or a negative GOL_E* code; the message
 *    is in gol_last_error(ctx).  No exception crosses the ABI.  (The reference
 *    has no error path beyond MPI_Abort, main.cpp:176-197.)
 *  - Host buffers are caller-owned 0/1 bytes, row-major, leading dimension
 *    `ld` (bytes).  Device memory is owned by the context.  On upload any
 *    nonzero byte is a live cell (cells are bools, main.cpp:73): it is stored,
 *    downloaded and counted as 1; bytes [ncols, ld) of a row are never read,
 *    and never written on download.
 *  - Coordinates are GLOBAL (row, col) of the rows×cols grid.
 *  - A context is not thread-safe; one host thread drives it.
 *  - gol_step is asynchronous (enqueues on the context's HIP streams);
 *    gol_sync / gol_download / gol_popcount synchronise.
 */
#ifndef GOLHIP_H
#define GOLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Cell layouts in HBM */
#define GOL_LAYOUT_BYTE 0 /* 1 byte per cell (0/1); row pitch = 256·n + 512 B (channel spread) */
#define GOL_LAYOUT_BIT 1  /* 1 bit per cell; column groups of G u32 words, column 32G·g+G·j+w in
                             word G·g+w, bit j (interleaved: neighbours share a bit); G = 4 for
                             tblock_k >= 8 (8, 16, 32), else 2.  Never visible through this ABI (host I/O is
                             0/1 bytes) */

/* Boundary conventions */
#define GOL_DEAD 0          /* non-periodic (main.cpp, P=1; periods {0,0} main.cpp:243): everything
                               outside the grid is permanently dead; it does not evolve, whatever the
                               rule (gol_set_rule), which is why B0 rules are refused */
#define GOL_SERIAL_COMPAT 1 /* main_serial.cpp:45-71: DEAD on the top-left (n-1)², last row/col 0 */
#define GOL_MESH_COMPAT 2   /* main.cpp on a √P×√P mesh, P=mesh_m²: swapped column halos
                               (main.cpp:51-54); any layout and tblock_k (stored as a dead-boundary
                               board with its column blocks in reverse order) */
#define GOL_TORUS 3         /* periodic B3/S23 (the other value of main.cpp:243's periods): row -1 is
                               row rows-1, column -1 is column cols-1.  Any layout, tblock_k = K and
                               slab count with cols >= K and every slab (a single one too) >= K
                               rows; mesh_m is ignored.  Stored with K ghost columns per side that a
                               wrap kernel refreshes after every launch, and the halo exchange closed
                               into a ring; gol_init_glibc: GOL_INIT_STREAM only (the cells of a
                               GOL_DEAD board of that size and seed) */

/* Seeded initialisation (glibc rand()%3==0, main.cpp:73 / main_serial.cpp:40) */
#define GOL_INIT_STREAM 0 /* srand(seed), row-major over the global grid (MPI np=1 with seed 0≡1) */
#define GOL_INIT_SERIAL 1 /* main_serial.cpp:34-43 with srand(seed): cell (r,c) ← draw (r+1)·n+c+1 */
#define GOL_INIT_MESH 2   /* main.cpp:68-77: block (cx,cy) ← srand(seed + cx·m + cy) */
#define GOL_SERIAL_SEED 1804289383u /* glibc's first rand() with no srand (main_serial.cpp:150) */

/* Halo transports */
#define GOL_XPORT_NONE 0 /* one slab */
#define GOL_XPORT_PEER 1 /* several slabs in this process: hipMemcpyAsync D2D / peer over xGMI */
#define GOL_XPORT_RCCL 2 /* one slab per process: ncclSend/ncclRecv over xGMI */

/* Error codes */
#define GOL_OK 0
#define GOL_EINVAL (-1)
#define GOL_EHIP (-2)
#define GOL_ERCCL (-3)
#define GOL_ENOMEM (-4)
#define GOL_EUNSUPPORTED (-5)
#define GOL_ESTATE (-6)

#define GOL_UNIQUE_ID_BYTES 128

/* gol_set_option keys */
#define GOL_OPT_CHUNK_ROWS 1    /* rows per wave chunk; -r: exactly r rounds of resident waves;
                                   -(100+r): guided static schedule, r rounds of halving chunks.
                                   0 (0.1's work queue) is GOL_EUNSUPPORTED since 0.2.
                                   Setting it turns off the bit k=8 schedule trial; reading it
                                   returns the policy in force (the trial's pick once known) */
#define GOL_OPT_KERNEL_TIMING 2 /* 1: bracket every main-kernel launch with hipEvents (at most 1024
                                   pairs in flight; older ones are harvested as new ones are needed) */
#define GOL_OPT_WORDS_PER_LANE 3 /* retired in 0.2 (lane widths are fixed per kernel): set is a no-op */
#define GOL_OPT_OVERLAP 4       /* multi-slab: 1 = interior kernel overlapped with halo exchange (default) */
#define GOL_OPT_BYTE_CORE 5     /* byte layout: 1 = bit-sliced core where tblock_k is 4, 8, 12, 16, 20,
                                   24, 28, 32, 48, 56 or 64 (default; the kernel per depth is the library's
                                   pick); 2 = its one-wave-per-strip kernel (k <= 32); 3 = its chain
                                   kernel (a workgroup of 2-4 waves per strip splitting the stages,
                                   k = 24, 32, 48, 64; 48 and 64 always run it); 4 = the byte board
                                   through the bit board's pair waves (a pack wave, k / 8 pair waves,
                                   an unpack wave per strip; k = 16, 24, 32, 48, 56, other depths as 1);
                                   0 = byte-SWAR kernel (tblock_k <= 8) */
#define GOL_OPT_SPLIT 6         /* retired in 0.2 (boundary bands are always split off): set is a no-op */
#define GOL_OPT_TEXT_BLOCK_BYTES 10 /* snapshot text: bytes per pinned staging block (default 64 MiB) */
#define GOL_OPT_SCHEDULE_TRIAL 11 /* bit layout, tblock_k = 8, no caller chunk policy: 1 (default) = after
                                     400 k-steps, time the policies -1/-2/-3 (split interior, the k = 8
                                     default) or -104/-6/-3 (unsplit) on 24 real steps (results are
                                     unaffected) and keep the fastest (the default -1 resp. -104 unless
                                     another is > 4 % resp. 1.5 % faster); never blocks the host (the
                                     pick applies once its events have completed); 0 = off.  Reads 2
                                     once the pick is made.  RCCL mode: 16 k-steps after the trial the
                                     ranks take the MAX of their medians (ncclAllReduce on the context's
                                     communicator, the same k-step on every rank) and all keep the same
                                     policy; a short k-step during the trial restarts it.  RCCL mode:
                                     this option and GOL_OPT_CHUNK_ROWS are COLLECTIVE before the trial
                                     starts (set them alike on every rank before k-step 400, or a rank
                                     without the trial leaves the others in the allreduce); set on one
                                     rank once the trial is recording, they do not take that rank out
                                     of it: it joins the agreement and then keeps its own setting */

#define GOL_OPT_INTERIOR_SPLIT 12 /* P = 1 .. 4: a slab's interior runs as P launches on P streams
                                     with a 2k-row seam band at every cut on the halo stream, so the
                                     next step's parts start while this step's parts drain (a slab
                                     takes the most parts with >= 32·tblock_k interior rows each,
                                     down to one).
                                     Default 2 for bit layout at tblock_k >= 8 (8, 16, 32) with at most 4 slabs per
                                     device whose 3 streams each (+ the clock probe's) fit the process's
                                     hardware queues (3 x slabs + 1 <= GPU_MAX_HW_QUEUES, HIP default 4:
                                     one slab per device), 1 otherwise.  Setting it synchronises the context; with no
                                     caller chunk policy the k = 8 default policy follows it (-1 split,
                                     -104 unsplit) and a trial under way starts over.  RCCL mode: like
                                     GOL_OPT_SCHEDULE_TRIAL, collective before the trial starts; set on
                                     one rank while the trial records, the rank's slots keep timing
                                     the trial's candidates, it joins the agreement, and then keeps
                                     the new split's default policy */

#define GOL_OPT_SCHED_TRACE 13  /* diagnostic: 1 = record the enqueue order of the step path (event
                                   records and waits, host syncs, board reads/writes per stream) for
                                   gol_sched_trace; setting it clears the record */

#define GOL_OPT_COMM_TIMING 14  /* multi-slab / RCCL mode: 1 = time each local slab's comm-stream work
                                   per k-step with hipEvents — the halo exchange (ncclSend/Recv group or
                                   peer copies) and the boundary + seam bands — read by gol_comm_time */

#define GOL_OPT_HALO_EXCHANGE 15 /* diagnostic: 0 = skip the halo exchange (no rows move between slabs,
                                    so results at slab seams are WRONG): the same slabs, bands and
                                    interior launches without communication, for an interior-only step
                                    time beside the real one (bench.py's N > 1 line); 1 = default.
                                    RCCL mode: collective (set it alike on every rank) */

#define GOL_OPT_RULE_KERNEL 16  /* 0 (default): B3/S23 runs the tuned kernels; 1: every rule, B3/S23 too,
                                   runs the rule-generic kernel (a context gol_set_rule supports; others
                                   GOL_EUNSUPPORTED).  Setting it synchronises the context.  RCCL mode:
                                   local state, results do not depend on it */

#define GOL_OPT_RULE_COMPILED 17 /* 1 (default): a rule on the list of gol_compiled_rule runs the kernel
                                    compiled for it, at a depth that has one; 0: it runs the rule-generic
                                    kernel like any other rule.  GOL_OPT_RULE_KERNEL = 1 takes precedence
                                    (everything generic).  Values other than 0 and 1 are GOL_EINVAL.
                                    Setting it synchronises the context.  RCCL mode: local state,
                                    results do not depend on it */

/* gol_rule_path: which kernels the next gol_step launches for the context's rule. */
#define GOL_RULE_PATH_TUNED 0    /* B3/S23 on the kernels tuned for it */
#define GOL_RULE_PATH_GENERIC 1  /* the rule-generic kernel (the rule is a launch argument) */
#define GOL_RULE_PATH_COMPILED 2 /* the kernel compiled for this rule (the rule is its immediates) */

typedef struct gol_ctx gol_ctx;

/* Single process.  The grid is cut into n_gpus row slabs; slab s lives on HIP
 * device s % (visible devices), so n_gpus > devices exercises the multi-slab
 * path on one GPU.  tblock_k = generations fused per launch and halo depth.
 * Replaces MPI_Init/Dims_create/Cart_create (main.cpp:154-254). */
int gol_create(gol_ctx **out, int64_t rows, int64_t cols, int n_gpus, int layout, int boundary,
               int mesh_m, int tblock_k);

/* One process per GPU (torchrun-style).  This context owns slab `rank` of
 * `world` on HIP device `device`; halos go over RCCL.  `unique_id` is the
 * GOL_UNIQUE_ID_BYTES blob from gol_get_unique_id() on rank 0, broadcast by
 * the caller.  Replaces MPI_Init/Cart_create/Cart_shift (main.cpp:154-254). */
int gol_create_rank(gol_ctx **out, int64_t rows, int64_t cols, int rank, int world, int device,
                    const uint8_t *unique_id, int layout, int boundary, int mesh_m, int tblock_k);
int gol_get_unique_id(uint8_t *unique_id);

/* Row range of slab `rank` of `world` (host-only arithmetic, no GPU needed). */
int gol_slab_plan(int64_t rows, int world, int rank, int64_t *row0, int64_t *nrows);

int gol_set_option(gol_ctx *ctx, int option, int64_t value);
int gol_get_option(gol_ctx *ctx, int option, int64_t *value);

/* Life-like (outer-totalistic) rules in B/S notation.  Bit n (0..8) of `birth`: a
 * dead cell with n live neighbours, out of 8, is born; bit n of `survive`: a live
 * cell with n live neighbours stays alive.  A new context runs B3/S23
 * (birth = 1<<3, survive = (1<<2)|(1<<3)), the one rule the reference knows
 * (main.cpp:79-91), on the kernels tuned for it; a rule on the list of
 * gol_compiled_rule runs a kernel compiled for it (GOL_OPT_RULE_COMPILED); any
 * other rule runs the rule-generic kernel.  All three compute the same boards.
 *   gol_parse_rule  (host only, no context) "B36/S23" or "S23/B36" in either letter
 *                   case, or the legacy survive/birth form "23/3"; a digit list may
 *                   be empty ("B2/S"); digits are 0..8, each at most once.  Anything
 *                   else is GOL_EINVAL.  It does not judge the rule (B0 parses).
 *   gol_set_rule    any time between steps; synchronises the context (as
 *                   GOL_OPT_INTERIOR_SPLIT does) and holds from the next gol_step.
 *                   GOL_EINVAL: bits above 8, or B0 (birth & 1) — cells outside the
 *                   grid, pad columns and rows outside a slab's live rows are dead at
 *                   every generation, and the runtime relies on dead staying dead in
 *                   empty space.  A rule other than B3/S23 (and GOL_OPT_RULE_KERNEL = 1)
 *                   needs GOL_LAYOUT_BIT, tblock_k 1..7 (2-word groups), GOL_DEAD or
 *                   GOL_TORUS; any slab count, either transport.  GOL_EUNSUPPORTED
 *                   naming the limit otherwise: the byte layout, tblock_k >= 8, and
 *                   GOL_SERIAL_COMPAT / GOL_MESH_COMPAT (they reproduce the reference
 *                   program, which knows one rule); the context stays usable.
 *                   Setting B3/S23 itself is GOL_OK on every context.
 *                   RCCL mode: the rule is local state, so the call is COLLECTIVE:
 *                   set it alike on every rank, between the same two steps.
 *   gol_get_rule    the rule in force.
 *   gol_compiled_rule (host only, no context) entry `index` (0, 1, ...) of the list of
 *                   rules with kernels of their own: its masks and its usual name
 *                   (a static string).  Any output may be null.  An index outside
 *                   the list is GOL_EINVAL, so counting up to the first GOL_EINVAL
 *                   enumerates it.  B3/S23 is not on it.
 *   gol_rule_path   what the next gol_step of this context launches for its rule, one
 *                   of GOL_RULE_PATH_*: the rule in force, GOL_OPT_RULE_KERNEL and
 *                   GOL_OPT_RULE_COMPILED decide it, in that order (tuned, else
 *                   compiled, else generic).  A short last block of a step may run
 *                   a shallower kernel of the same or the generic path. */
int gol_parse_rule(const char *text, uint32_t *birth, uint32_t *survive);
int gol_set_rule(gol_ctx *ctx, uint32_t birth, uint32_t survive);
int gol_get_rule(gol_ctx *ctx, uint32_t *birth, uint32_t *survive);
int gol_compiled_rule(int index, uint32_t *birth, uint32_t *survive, const char **name);
int gol_rule_path(gol_ctx *ctx, int *path);

/* On-device glibc-rand initialisation with jump-ahead, bit-identical to the
 * reference's initializeBoard (main.cpp:68-77, main_serial.cpp:34-43). */
int gol_init_glibc(gol_ctx *ctx, int mode, uint32_t seed);

/* Host 0/1 bytes → device (whole grid / a window).  For a rank context only
 * the rows of its slab are taken.  Cells outside the active region of the
 * boundary convention (SERIAL_COMPAT: last row and column) are stored as 0. */
int gol_upload(gol_ctx *ctx, const uint8_t *host, int64_t ld);
int gol_upload_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                      const uint8_t *host, int64_t ld);

/* Advance `generations` generations: updateBoard + pointer swap + distr_borders
 * of main.cpp:291-305, `tblock_k` generations per launch and per halo exchange. */
int gol_step(gol_ctx *ctx, int64_t generations);

/* Wait for all enqueued work.  elapsed_ms (may be NULL) = device time from the
 * first gol_step after the previous sync to completion (hipEvents). */
int gol_sync(gol_ctx *ctx, double *elapsed_ms);

/* Device → host 0/1 bytes (whole grid / a window; rank contexts: own slab rows only). */
int gol_download(gol_ctx *ctx, uint8_t *host, int64_t ld);
int gol_download_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                        uint8_t *host, int64_t ld);
/* Asynchronous window copy: enqueued behind every gol_step so far (no host
 * wait, no device idle); `host` (caller-owned, valid until then) is filled by
 * the next synchronising call (gol_sync, gol_popcount, gol_download*, ...).
 * Rows must be held by this context.  Snapshot-at-a-generation without a
 * pipeline drain (bench.py takes its verification cone this way). */
int gol_download_window_async(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                              uint8_t *host, int64_t ld);

/* 1-bit-per-cell board I/O: the calls above with packed rows, an eighth of the
 * bytes on every transfer.  Row i of the window starts at host + i*ld (ld in
 * BYTES, ld >= gol_bits_row_bytes(ncols) = (ncols + 7) / 8); column col0 + j is bit
 * 7 - (j & 7) of byte j >> 3 of its row, MSB first, 1 = live: numpy's
 * packbits(window, axis=1) and the raster of a PBM `P4` image.  The format is
 * defined on bytes (no endianness); col0 and ncols are arbitrary.  The packing runs
 * on the device; the result equals packbits of what gol_download[_window] returns,
 * for every layout, group width, tblock_k, boundary storage (torus ghost columns,
 * MESH_COMPAT's reversed blocks), slab count and transport.
 *   download: the 8*row_bytes - ncols pad bits of a row's last byte are written as
 *             0; bytes [row_bytes, ld) of a row are not touched.
 *   upload:   pad bits are ignored; only the window's cells change; cells outside
 *             the active region (SERIAL_COMPAT: last row and column) are stored as 0.
 * Rank contexts move the rows they hold, as the byte calls do; the _async form
 * needs every row held, is enqueued behind every gol_step so far and is delivered
 * by the next synchronising call (a failed call leaves no pending write).  Staging
 * comes from the context's pool (see gol_clock_start).  GOL_EINVAL with a message:
 * window outside the grid, ld too small, a null buffer.  An empty window is GOL_OK
 * and writes nothing.  gol_bits_row_bytes: host only; ncols < 0 gives GOL_EINVAL.
 * No reference counterpart. */
int64_t gol_bits_row_bytes(int64_t ncols);
int gol_download_bits(gol_ctx *ctx, uint8_t *host, int64_t ld);
int gol_download_bits_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                             uint8_t *host, int64_t ld);
int gol_download_bits_window_async(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                                   uint8_t *host, int64_t ld);
int gol_upload_bits(gol_ctx *ctx, const uint8_t *host, int64_t ld);
int gol_upload_bits_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                           const uint8_t *host, int64_t ld);

/* Random fill: a seeded soup at any density, written where the board lives — no
 * host array, no PCIe.  Counter-based: every cell is a formula of (seed, threshold,
 * GLOBAL row, GLOBAL column).  All arithmetic mod 2^64, sm = splitmix64's output
 * function exactly as under gol_digest:
 *   K        = sm(seed)                                  seed: uint64
 *   h(r,w,j) = sm( sm(K + r) + 16*w + j )                r = global row, w = global column >> 5, j = 0..15
 *   plane 2j   (r,w) = low  32 bits of h(r,w,j)
 *   plane 2j+1 (r,w) = high 32 bits of h(r,w,j)
 *   X(r,c)   = sum over i = 0..31 of 2^i * bit (c & 31) of plane i (r, c >> 5)      (uniform in [0, 2^32))
 *   cell (r,c) is live  iff  X(r,c) < T                  T: uint64 threshold, 0 <= T <= 2^32
 * T = 0 clears the window, T = 2^32 sets every cell, the density is T / 2^32.  A
 * cell depends on (seed, T, r, c) only: not on the window, the layout, the group
 * width, tblock_k, the boundary storage, the slab or the rank that writes it, so a
 * window fill equals the same cells of a whole-board fill and the parts of rank
 * contexts tile the board's fill with no communication.  Planes below the lowest set
 * bit of T cannot decide X < T and are not computed: density 1/2 costs half an sm
 * per 32 cells, a full 32-bit threshold 16.  Not cryptographic.  No reference
 * counterpart (gol_init_glibc is the reference's start: density 1/3 only).
 *   gol_fill_threshold      host only: *threshold = llround(density * 2^32) for
 *                           0 <= density <= 1; GOL_EINVAL for NaN, a value outside
 *                           [0, 1], a null pointer.
 *   gol_fill_random_window  behaves as an upload: it writes the current buffer, only
 *                           the window's cells change, the generation, the rule and
 *                           the schedule trial stay untouched; it synchronises before
 *                           and after the write.  A rank context writes the rows it
 *                           holds.  Cells outside the active region (SERIAL_COMPAT:
 *                           last row and column) are stored as 0; torus ghost columns
 *                           are refreshed.  GOL_EINVAL with a message: a window outside
 *                           the grid, threshold > 2^32.  An empty window is GOL_OK and
 *                           writes nothing.  Nothing is allocated or staged (see
 *                           gol_clock_start).
 *   gol_fill_random         the whole grid; a rank context: its slab. */
int gol_fill_threshold(double density, uint64_t *threshold);
int gol_fill_random(gol_ctx *ctx, uint64_t seed, uint64_t threshold);
int gol_fill_random_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                           uint64_t seed, uint64_t threshold);

/* Board-to-board copies, on the device: the cells of a window of `src` are merged
 * into a window of the same size of `dst`.  In LOGICAL cells (global coordinates,
 * as gol_download shows them): for 0 <= i < nrows and 0 <= j < ncols, cell
 * (drow0 + i, dcol0 + j) of dst becomes op(its old value, cell (srow0 + i, scol0 + j)
 * of src); no other cell of dst changes and src does not change.  The two contexts
 * need not agree in anything: layout and group width, tblock_k, boundary storage
 * (torus ghost columns, MESH_COMPAT's reversed blocks: ghost columns are never
 * copied as cells), slab count, transport and size are each side's own; one kernel
 * goes from storage to storage in one pass, at any column shift.
 *   gol_copy_window  behaves as an upload into dst: it writes dst's current buffer;
 *                    the generation, rule, options and schedule trial of both
 *                    contexts stay as they are; cells outside dst's active region
 *                    (SERIAL_COMPAT: last row and column) are stored as 0 under every
 *                    op; dst's torus ghost columns are refreshed.  It synchronises
 *                    both contexts before the write and dst after it (pending async
 *                    windows, digests and maps of both are delivered).  Nothing is
 *                    allocated or staged (see gol_clock_start).
 *                    Rank contexts: the rows of the destination window that dst
 *                    holds are written, the others are skipped; every written row's
 *                    source row must be held by src.
 *                    src == dst is allowed when the two rectangles are disjoint (a
 *                    pattern tiled within one board).
 *                    Errors are found before anything is written (dst is unchanged),
 *                    the message goes to gol_last_error(dst).  GOL_EINVAL: a null
 *                    context (no message); a window outside either grid; negative
 *                    sizes; an unknown op; a source row that src does not hold; a
 *                    destination window with no local rows unless dst is a rank
 *                    context; overlapping rectangles in one context.
 *                    GOL_EUNSUPPORTED: a row piece whose source slab and destination
 *                    slab live on different HIP devices — this version copies
 *                    within a device (two contexts of the same n_gpus and rows line
 *                    up slab for slab).  An empty window is GOL_OK and writes nothing.
 *   gol_copy         the whole board, REPLACE; GOL_EINVAL unless rows and cols match.
 *                    Rank contexts: the rows dst holds.
 * There is no _async form in this version: ordering the streams of two contexts
 * against each other is a piece of work of its own.  No reference counterpart. */
#define GOL_COPY_REPLACE 0   /* dst = src            */
#define GOL_COPY_OR      1   /* dst = dst | src      */
#define GOL_COPY_XOR     2   /* dst = dst ^ src      */
int gol_copy_window(gol_ctx *dst, int64_t drow0, int64_t dcol0,
                    gol_ctx *src, int64_t srow0, int64_t scol0,
                    int64_t nrows, int64_t ncols, int op);
int gol_copy(gol_ctx *dst, gol_ctx *src);

/* Snapshot text —the body of a `.gol` part file as writeBoardToFile writes it
 * (main.cpp:106-129, main_serial.cpp:74-95; read back by
 * gol_visualization.py:29-33): for every row of the window one "0\t" or "1\t"
 * per cell, then "\n".  The two header lines ("firstRow lastRow" /
 * "firstCol lastCol") stay with the caller.  Formatting and parsing run on the
 * device; the host moves finished bytes (pipelined through pinned buffers).
 * Every row of the window must be held by this context (a rank writes its own
 * part, as in the reference).
 *   gol_text_bytes   bytes of an nrows×ncols body: nrows·(2·ncols+1)
 *   gol_format_text  body → caller memory (out_len >= gol_text_bytes)
 *   gol_write_text   body → file descriptor (write(2), sequential)
 *   gol_parse_text   caller memory (exactly gol_text_bytes) → cells (snapshot resume)
 *   gol_read_text    file descriptor (read(2), positioned at the body) → cells
 * Malformed text (any byte other than the pattern above) is GOL_EINVAL with
 * the offending offset in gol_last_error; the window may then be partly
 * written.  No reference counterpart reads snapshots back. */
int64_t gol_text_bytes(int64_t nrows, int64_t ncols);
int gol_format_text(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, char *out,
                    int64_t out_len);
int gol_write_text(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int fd);
int gol_parse_text(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, const char *text,
                   int64_t len);
int gol_read_text(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int fd);

/* RLE pattern text — the run-length format of Life pattern collections:
 *     x = <ncols>, y = <nrows>, rule = B<digits>/S<digits>\n
 *     24bo$22bobo$...!\n
 * A token is an optional count n >= 2 and a tag: b (dead run), o (live run),
 * $ (end of row), ! (end of pattern).  WRITING is canonical ("RLE
 * pattern files"): the rule is the context's (gol_get_rule), a row's runs end at
 * its last live cell, empty rows fold into the next `$` count, trailing empty
 * rows are left to `y`; with L = 70 / (1 + D), D the decimal digits of
 * max(nrows, ncols, 1), a '\n' follows every L-th token and `!`, so no line
 * exceeds 70 characters.  The text is encoded on the device from the window's
 * logical cells (what gol_download_window returns), in blocks of rows whose worst
 * case fits GOL_OPT_TEXT_BLOCK_BYTES; only the text crosses PCIe.  Every row of
 * the window must be held by this context, as for snapshot text; GOL_ESTATE while
 * the clock probe runs.  An empty window (nrows = 0 or ncols = 0) is its header
 * and "!\n".
 *   gol_rle_header  host only, no context: the header line of an RLE text (after any
 *                   '#' lines).  *body = offset of the first body byte.  *has_rule = 0
 *                   and B3/S23 in the masks when the header names no rule.  Out
 *                   pointers may be NULL.  Malformed: GOL_EINVAL.
 *   gol_rle_bytes   bytes of the window's RLE, header included (row pass + row scan
 *                   only; synchronises)
 *   gol_format_rle  text → caller memory; cap too small: GOL_EINVAL, *len = bytes
 *                   needed, contents of out unspecified
 *   gol_write_rle   text → file descriptor (write(2), sequential)
 * READING accepts more than writing produces: leading '#' lines, free spacing in
 * the header (`x=3,y=3`), an optional `rule = ...` in any notation gol_parse_rule
 * reads, white space (space, tab, \r, \n) between tokens, anything after `!`.
 *   gol_parse_rle   header + body from memory; the pattern's top-left cell goes to
 *                   (row0, col0); x, y (may be NULL) = its box
 *   gol_read_rle    the same from a file descriptor (read(2), in chunks)
 * The x × y box at (row0, col0) is REPLACED, cells outside it do not change; a box
 * that leaves the grid, or rows that are not all held, is GOL_EINVAL before anything
 * is written; x = 0 or y = 0 reads as GOL_OK and writes nothing.  The header's rule
 * is NOT set (gol_rle_header + gol_set_rule is the caller's decision).  Malformed
 * text is GOL_EINVAL with the byte offset in gol_last_error: a rule gol_parse_rule
 * refuses, any byte that is no count, tag or white space (the multi-state tags `.`
 * and A..X among them), white space between a count and its tag, a count of 0 or
 * above 2^31, a run or row that leaves the box, the end of input before `!`; the
 * box may then be partly written.  The generation, the rule, the options and the
 * schedule trial stay untouched by all six calls. */
int gol_rle_header(const char *text, int64_t len, int64_t *x, int64_t *y,
                   uint32_t *birth, uint32_t *survive, int *has_rule, int64_t *body);
int gol_rle_bytes(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int64_t *bytes);
int gol_format_rle(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                   char *out, int64_t cap, int64_t *len);
int gol_write_rle(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int fd);
int gol_parse_rle(gol_ctx *ctx, int64_t row0, int64_t col0, const char *text, int64_t len,
                  int64_t *x, int64_t *y);
int gol_read_rle(gol_ctx *ctx, int64_t row0, int64_t col0, int fd, int64_t *x, int64_t *y);

/* Live cells held by this context (all its slabs). */
int gol_popcount(gol_ctx *ctx, int64_t *live);

/* Board digest: 128 bits (two 64-bit lanes) of the LOGICAL board, computed where
 * the board lives — "is this board the same as that one?", "has it started
 * repeating?" without a download.  All arithmetic mod 2^64:
 *   sm(x):  z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)    (splitmix64)
 *   A_i(r) = sm(4r + i) | 1,  B_i(w) = sm(4w + 2 + i) | 1,  i = 0, 1
 *   digest[i] = sum over the live cells (r, c) of A_i(r) * B_i(c >> 5) * 2^(c & 31)
 * with GLOBAL (r, c).  It is the same for every layout, group width, tblock_k,
 * boundary storage (torus ghost columns, MESH_COMPAT's reversed blocks), slab count
 * and transport: it equals the digest of what gol_download returns, in every state
 * (GOL_SERIAL_COMPAT: the inactive last row and column are stored as 0).  The empty
 * board gives (0, 0); digests of disjoint windows ADD (mod 2^64), so rows this
 * context does not hold contribute nothing and the parts of rank contexts add up to
 * the board's digest (no collective is involved; the caller adds).  Two boards that
 * differ inside one aligned 32-column word of one row always differ in both lanes;
 * any other difference is caught with probability ~1 - 2^-64 per lane.  Not
 * cryptographic.  No reference counterpart.
 *   gol_digest         whole grid; synchronises.
 *   gol_digest_window  a window; synchronises.  A window outside the grid is GOL_EINVAL.
 *   gol_digest_async   whole grid, enqueued behind every gol_step so far (no host wait,
 *                      no device idle); `digest` (caller-owned, valid until then) is
 *                      filled by the next synchronising call, as the windows of
 *                      gol_download_window_async are.  At most 1024 may be pending per
 *                      context: one more is GOL_ESTATE (sync first).  A failed call
 *                      leaves no pending write.
 * The digest slots are allocated at the first call of any of the three; while a clock
 * probe runs nothing is allocated (gol_clock_start), so a context that has taken no
 * digest yet returns GOL_ESTATE: take one beforehand. */
int gol_digest(gol_ctx *ctx, uint64_t digest[2]);
int gol_digest_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                      uint64_t digest[2]);
int gol_digest_async(gol_ctx *ctx, uint64_t digest[2]);

/* Density map: per-tile live-cell counts of the LOGICAL board, computed where the
 * board lives — a coarse view of a board nobody can download (where the live cells
 * are, where a soup has died out or grows).  The window [row0, row0 + nrows) ×
 * [col0, col0 + ncols) is cut into tiles of tile_rows × tile_cols cells from its
 * origin: *trows = ceil(nrows / tile_rows), *tcols = ceil(ncols / tile_cols)
 * (gol_density_dims: host only, no context; GOL_EINVAL for null pointers, a negative
 * size or a tile size < 1).
 *   counts[i*ld + j] = the number of live cells (r, c) with
 *       row0 + i*tile_rows <= r < min(row0 + (i+1)*tile_rows, row0 + nrows)
 *       col0 + j*tile_cols <= c < min(col0 + (j+1)*tile_cols, col0 + ncols)
 * with GLOBAL (r, c); `ld` is in elements and must be >= tcols.  Tiles of the last
 * tile row and tile column are clipped to the window.  The map equals the map of
 * what gol_download returns, in every state, for every layout, group width,
 * tblock_k, boundary storage, slab count and transport: torus ghost columns and
 * halo rows are never counted, MESH_COMPAT maps are in logical columns, and
 * GOL_SERIAL_COMPAT's inactive last row and column count 0.  Maps ADD: rows this
 * context does not hold contribute 0 to every tile, the whole trows × tcols block of
 * `counts` is always written, and the maps of rank contexts add up to the board's
 * map (no collective is involved; the caller adds).
 * GOL_EINVAL (message in gol_last_error): a window outside the grid, tile_rows < 1,
 * tile_cols < 32 or not a multiple of 32, col0 not a multiple of 32,
 * tile_rows*tile_cols > 2^32 - 1 (a count is 32 bits), ld < tcols, null pointers;
 * a refused call writes nothing to `counts`, and elements [tcols, ld) of a row are
 * never written.  The multiple-of-32 rule is deliberate in this version: every
 * aligned 32-column word of a row then belongs to exactly one tile.  An empty window
 * (nrows == 0 or ncols == 0) is GOL_OK and writes nothing.
 *   gol_density         whole grid; synchronises.
 *   gol_density_window  a window; synchronises.
 *   gol_density_async   whole grid, enqueued behind every gol_step so far (no host
 *                       wait, no device idle); `counts` (caller-owned, valid until
 *                       then) is filled by the next synchronising call, as the windows
 *                       of gol_download_window_async are.  A failed call leaves no
 *                       pending write.
 * The per-slab parts live in the context's pooled staging, as window copies do (see
 * gol_clock_start).  No reference counterpart. */
int gol_density_dims(int64_t nrows, int64_t ncols, int64_t tile_rows, int64_t tile_cols,
                     int64_t *trows, int64_t *tcols);
int gol_density(gol_ctx *ctx, int64_t tile_rows, int64_t tile_cols, uint32_t *counts, int64_t ld);
int gol_density_window(gol_ctx *ctx, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                       int64_t tile_rows, int64_t tile_cols, uint32_t *counts, int64_t ld);
int gol_density_async(gol_ctx *ctx, int64_t tile_rows, int64_t tile_cols, uint32_t *counts, int64_t ld);

/* Generations advanced so far. */
int gol_generation(gol_ctx *ctx, int64_t *generation);

/* With GOL_OPT_KERNEL_TIMING: summed device time (ms) and count of main-kernel
 * launches since the last reset (the hot kernel's average = total / count).
 * Without it: total 0 and the launch count (counted on the host). */
int gol_kernel_time(gol_ctx *ctx, double *total_ms, int64_t *launches, int reset);

/* With GOL_OPT_COMM_TIMING: device time (ms) the comm stream spent in the halo
 * exchange (*exchange_ms) and in the boundary and seam bands (*bands_ms), summed
 * over *steps k-steps since the last reset, for the local slab whose sum is
 * largest.  Synchronises.  The halo path of main.cpp:291-305 (distr_borders,
 * main.cpp:36-65, plus the per-generation MPI_Barrier) is what this times. */
int gol_comm_time(gol_ctx *ctx, double *exchange_ms, double *bands_ms, int64_t *steps, int reset);

/* Diagnostic (GOL_OPT_SCHED_TRACE): *n = ops recorded; with ops != NULL and
 * cap >= *n, copies them (7 int64 each: kind 1 record / 2 wait / 3 stream sync
 * / 4 event sync / 5 read / 6 write, stream, event, slab, buffer, row0, row1 —
 * storage rows, all columns) and clears the record.  The record holds at
 * most 2^22 ops; past that GOL_ESTATE (set the option again to restart it).  A happens-before check of
 * the streams' order, the event edges and the host syncs over these ops finds
 * any two accesses of the same rows, one a write, left unordered
 * (tests/sched_race.py).  Reference analogue: none (the MPI code is blocking). */
int gol_sched_trace(gol_ctx *ctx, int64_t *ops, int64_t cap, int64_t *n);

/* Clock probe (measurement): gol_clock_start launches a one-wave kernel on a
 * stream of its own that stamps the shader-clock counter (s_memtime) and the
 * 100-MHz real-time counter, sleeps between polls of a host flag, and stops at
 * gol_clock_stop or after max_ms.  mhz = shader cycles / real time over that
 * span: the clock the chip ran at while the enqueued steps executed (the
 * probe itself holds one wave slot of one CU).  While it runs nothing is
 * allocated on the device: window copies (gol_download_window[_async],
 * gol_upload_window) use the context's pooled staging (GOL_ESTATE if no pooled
 * buffer of the size is free: copy one window of that size beforehand; the
 * parts of gol_density* come from the same pool under the same rule: take one
 * map with the same window and tiles beforehand), and
 * the snapshot-text calls and gol_init_glibc return GOL_ESTATE; gol_digest* need
 * their slots allocated by an earlier digest (GOL_ESTATE otherwise).
 * gol_fill_random[_window] allocates and stages nothing: it works while the probe
 * runs.  So does gol_copy[_window], with the probe on either context. */
int gol_clock_start(gol_ctx *ctx, double max_ms);
int gol_clock_stop(gol_ctx *ctx, double *mhz, double *span_ms);

/* Transport self-test (no context): a 1-rank RCCL communicator on `device`
 * (the library's own dlopen'ed RCCL binding, as gol_create_rank uses it) runs
 * `reps` groups of two ncclSend/ncclRecv pairs of `bytes` each to itself on a
 * non-blocking stream — the halo exchange of a rank with two neighbours — and
 * checks every byte.  us_per_round (may be NULL): device time per group.
 * msg (may be NULL): outcome text. */
int gol_rccl_selftest(int device, int64_t bytes, int reps, double *us_per_round, char *msg, int msg_len);

const char *gol_last_error(gol_ctx *ctx);
void gol_destroy(gol_ctx *ctx);

/* Library / build identification (e.g. "golhip gfx950"). */
const char *gol_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GOLHIP_H */
