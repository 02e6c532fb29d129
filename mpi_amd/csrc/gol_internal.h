// Internal interface between the runtime (gol_runtime.cpp) and the gfx950
// kernels (gol_kernels.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gol_rule.h"

namespace gol {

// Bit layout = interleaved groups of gw u32 words (gw = 2 or 4): a group holds
// 32·gw consecutive columns, column c lives in word gw·(c / 32gw) + c % gw,
// bit (c % 32gw) / gw.  In a group a cell's left and right neighbours are the
// same bit of the adjacent word (one funnel shift at the group ends only), so
// the wider the group, the fewer lane moves per word.  A context's group width
// is fixed at creation (bit_group_words: 4 for the k = 8 pair kernel, 2
// otherwise); rows are padded to whole 128-column blocks (4 words) either way.
constexpr int kGroupWords = 2;   // the width of every kernel but the k = 8 pair kernel's
__host__ __device__ inline int64_t bit_word(int64_t c, int gw) {
    const int lg = gw == 4 ? 2 : 1;
    return ((c >> (5 + lg)) << lg) + (c & (gw - 1));
}
__host__ __device__ inline int bit_pos(int64_t c, int gw) {
    const int lg = gw == 4 ? 2 : 1;
    return (int)((c & (32 * gw - 1)) >> lg);
}

// n <= 32 consecutive columns [c0, c0+n) of one bit-layout row as a u32 (bit i =
// column c0+i), and back (only those columns' bits change).  A group holds at
// least 64 columns, so the range touches at most two groups, and in each word
// the wanted columns are one contiguous bit field [lo, hi): bit b of word j of
// group g is column 32gw·g + gw·b + j.  (GOL_TORUS ghost margins: launch_wrap_cols.)
template <typename F>
__host__ __device__ inline void for_col_fields(int64_t c0, int n, int gw, F &&fn) {
    const int lg = gw == 4 ? 2 : 1;
    const int64_t gc = 32 * gw;
    for (int64_t g = c0 / gc; g <= (c0 + n - 1) / gc; ++g)
        for (int j = 0; j < gw; ++j) {
            const int64_t base = g * gc + j;   // the column of this word's bit 0
            const int64_t a = c0 - base, e = c0 + n - base;
            const int lo = a <= 0 ? 0 : (int)((a + gw - 1) >> lg);
            int hi = e <= 0 ? 0 : (int)((e + gw - 1) >> lg);
            if (hi > 32) hi = 32;
            if (lo < hi) fn(g * gw + j, lo, hi, (int)(base + (int64_t)lo * gw - c0));
        }
}
__host__ __device__ inline uint32_t row_get_cols(const uint32_t *row, int64_t c0, int n, int gw) {
    uint32_t v = 0;
    for_col_fields(c0, n, gw, [&](int64_t wi, int lo, int hi, int at) {
        const uint32_t w = row[wi];
        for (int b = lo; b < hi; ++b, at += gw) v |= ((w >> b) & 1u) << at;
    });
    return v;
}
__host__ __device__ inline void row_put_cols(uint32_t *row, int64_t c0, int n, int gw, uint32_t v) {
    for_col_fields(c0, n, gw, [&](int64_t wi, int lo, int hi, int at) {
        uint32_t m = 0, bits = 0;
        for (int b = lo; b < hi; ++b, at += gw) {
            m |= 1u << b;
            bits |= ((v >> at) & 1u) << b;
        }
        row[wi] = (row[wi] & ~m) | bits;
    });
}

// Geometry of one pipelined-stencil launch.  Rows are STORAGE rows of a slab
// buffer: [0,hk) top halo, [hk,hk+H) slab rows, [hk+H,hk+H+hk) bottom halo.
struct StencilArgs {
    const void *src;
    void *dst;
    int64_t pitch;      // row pitch in u32 words
    int nunits;         // u32 words per row that carry active cells (bit: whole 4-word groups) / dwords (byte)
    uint32_t last_mask; // byte layout: 0x01 per active cell byte of the last active dword
    int64_t active_cols; // bit layout: columns [0, active_cols) are live (masks per interleaved word)
    int row_lo, row_hi; // storage rows outside [row_lo,row_hi) are dead at every generation
    int out_r0, out_r1; // storage rows produced by this launch
    int chunk_rows;     // output rows per wave chunk (see plan_items in gol_kernels.hip)
    int gw;             // bit layout: words per column group (2 or 4)
};

// Bit layout: the group width of a context fusing K generations per launch.
int bit_group_words(int K);

// Bit layout, `gens` generations fused (1..8, or 16 / 32: the chain of pair
// waves on 4-word groups), a.gw-word groups.
bool bit_depth_supported(int gens);
hipError_t launch_bit_pipe(const StencilArgs &a, int gens, hipStream_t s);
// Bit layout, any life-like rule (gol_rule.h; B3/S23 too): the rule-generic
// pipeline, gens = 1..7 on 2-word groups.  A launch it cannot serve is an error.
bool bit_rule_supported(int gens, int gw);
hipError_t launch_bit_rule(const StencilArgs &a, int gens, const RuleMasks &rule, hipStream_t s);
// Bit layout, a rule of GOL_COMPILED_RULES (gol_rule.h) by its index: the same
// pipeline with the rule compiled into the stage's immediates.  A depth or an
// index without a compiled kernel is an error (the caller asks first).
bool bit_crule_supported(int gens, int gw, int rule_index);
hipError_t launch_bit_crule(const StencilArgs &a, int gens, int rule_index, hipStream_t s);
// Byte layout, `gens` generations fused (1 <= gens <= 8), 16 cells per lane.
hipError_t launch_byte_pipe(const StencilArgs &a, int gens, hipStream_t s);
// Byte layout with the bit-sliced core (bytebit_pipe_kernel): byte-per-cell in
// HBM, gens in {4, 8, ..., 32, 48, 64} generations fused per launch.
bool bytebit_supported(int gens);
// core: which bit-sliced kernel (GOL_OPT_BYTE_CORE): the default per depth, one
// wave per strip (bytebit_pipe_kernel, k <= 32) or a chain of waves per strip
// (bytebit_coop_kernel, k in {24, 32, 48, 64}; k = 48, 64 have only the chain).
enum { kByteCoreDefault = 1, kByteCoreWave = 2, kByteCoreChain = 3, kByteCorePair = 4 };
bool bytebit_chain_default(int gens);
hipError_t launch_bytebit_pipe(const StencilArgs &a, int gens, hipStream_t s, int core = kByteCoreDefault);

// glibc-rand initialisation: one "unit" = a run of `len` consecutive draws of
// one stream written to storage row `row` starting at column `col0`.
struct InitUnit {
    int64_t row;
    int32_t col0;
    int32_t len;
    uint32_t w[31]; // raw generator values x_o .. x_{o+30} at the unit's first draw
    uint32_t pad;
};
// mats: T jump matrices (31×31, row-major) A^{t·seg}, t = 0..T-1.
hipError_t launch_init_units(const InitUnit *units, int nunits, const uint32_t *mats, int T, int seg,
                             void *dst, int64_t pitch_bytes, int bit_layout, hipStream_t s);

// Linear init words (bit i = column 32w+i) -> gw-word groups, rows [r0, r0+nrows)
// of `blocks` 128-column blocks.
hipError_t launch_interleave_rows(const uint32_t *lin, uint32_t *out, int64_t pitch_words, int64_t r0,
                                  int64_t nrows, int64_t blocks, int gw, hipStream_t s);
// Layout conversion of a window (dst/src host-staging buffers are device memory).
hipError_t launch_pack_window(const uint8_t *bytes, int64_t ld, uint32_t *words, int64_t pitch_words,
                              int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                              int64_t active_cols, int gw, hipStream_t s);
hipError_t launch_unpack_window(const uint32_t *words, int64_t pitch_words, uint8_t *bytes, int64_t ld,
                                int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int gw, hipStream_t s);
// Snapshot text (main.cpp:106-129 writeBoardToFile body): per row, "0\t"/"1\t" per
// cell then "\n" — rowlen = 2·ncols + 1 bytes; logical column c is read from
// storage column phys(c) (perm_m > 1: MESH_COMPAT's reversed blocks of perm_L).  format: storage rows
// [srow0, srow0+nrows), columns [col0, col0+ncols) of a slab buffer (bit words
// or bytes, pitch in bytes) -> text.  parse: text -> 0/1 bytes (ld); *err
// (preset to ~0) receives err_base + the lowest offending byte offset (atomicMin).
// bit_gw: 0 = byte layout, else the bit layout's group width.
hipError_t launch_format_text(const void *buf, int64_t pitch_bytes, int bit_gw, int64_t srow0, int64_t col0,
                              int64_t nrows, int64_t ncols, int perm_m, int64_t perm_L, char *text, hipStream_t s);
hipError_t launch_parse_text(const char *text, int64_t nrows, int64_t ncols, uint8_t *cells, int64_t ld,
                             int64_t err_base, unsigned long long *err, hipStream_t s);

// Byte layout upload: every nonzero byte of the window becomes 1 (bool cells).
hipError_t launch_normalize_bytes(uint8_t *base, int64_t pitch_bytes, int64_t nrows, int64_t ncols, hipStream_t s);

// Clock probe: one wave stamps (s_memtime, s_memrealtime) at start and end into
// out[0..3]; it ends when *stop (host-visible) is nonzero or after max_ticks of
// the 100-MHz real-time counter.
hipError_t launch_clock_probe(unsigned long long *out, const int *stop, unsigned long long max_ticks, hipStream_t s);

// Live-cell count of storage rows [r0,r1), accumulated into *acc.
hipError_t launch_popcount(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1,
                           int64_t row_bytes, unsigned long long *acc, int bit_layout, hipStream_t s);

// ---- GOL_TORUS: rows of cols + 2·hk storage columns, real column c at c + hk ----
// Refresh both ghost margins of storage rows [r0, r1): left ghost [0, hk) <- the
// last hk real columns, right ghost [hk+cols, cols+2hk) <- the first hk real
// columns.  Only ghost cells are written.  bit_gw: 0 = byte layout, else the
// bit layout's group width (hk <= 32 there).
hipError_t launch_wrap_cols(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t cols, int hk,
                            int bit_gw, hipStream_t s);
// launch_interleave_rows for a torus row: linear column c of `lin` (c < ncols)
// lands at storage column c + shift of the gw-word groups; every other bit of
// the row's row_words words is stored as 0.
hipError_t launch_interleave_rows_shift(const uint32_t *lin, uint32_t *out, int64_t pitch_words, int64_t r0,
                                        int64_t nrows, int64_t row_words, int64_t ncols, int shift, int gw,
                                        hipStream_t s);
// Live-cell count of storage columns [c0, c1) of storage rows [r0, r1), added to *acc.
hipError_t launch_popcount_cols(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t c0,
                                int64_t c1, unsigned long long *acc, int bit_gw, hipStream_t s);

// ---- gol_digest*: the layout-independent board digest (gol_digest.h) ----
// Storage rows [r0, r1) × storage columns [pc0, pc0 + ncols) of a slab buffer,
// where storage row r0 is GLOBAL row grow0 and storage column pc0 is logical
// column lc0 (lc0 - pc0 is arbitrary: torus ghost margin, MESH_COMPAT runs, user
// windows): both lanes of the cells' digest are added into slot[0], slot[1].
// Exactly these cells are read as cells (partial first and last words are
// masked).  bit_gw: 0 = byte layout, else the bit layout's group width.
hipError_t launch_digest(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                         int64_t lc0, int64_t ncols, unsigned long long *slot, int bit_gw, hipStream_t s);

// ---- gol_density*: per-tile live-cell counts (gol_density.h) ----
// The same cells as launch_digest's: storage rows [r0, r1) × storage columns
// [pc0, pc0 + ncols), storage column pc0 being logical column lc0.  The window the
// tiles belong to starts at logical column col0 (a multiple of 32, <= lc0) and
// trow_off rows above storage row r0 (>= 0); tiles are tile_rows × tile_cols
// (tile_cols a multiple of 32).  The cell of tile (i, j) is counted into
// part[(i - ti_base) * tcols + j]; the part holds ntr tile rows of tcols counts and
// is only added to (the caller clears it).  A run that would touch a tile outside
// the part is hipErrorInvalidValue.
hipError_t launch_density(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t trow_off, int64_t pc0,
                          int64_t lc0, int64_t ncols, int64_t col0, int64_t tile_rows, int64_t tile_cols,
                          uint32_t *part, int64_t ti_base, int64_t ntr, int64_t tcols, int bit_gw, hipStream_t s);

// ---- gol_download_bits* / gol_upload_bits*: 1-bit-per-cell rows (gol_bits.h, gol_bits.hip) ----
// launch_digest's cells: storage rows [r0, r1) × storage columns [pc0, pc0 + ncols),
// storage column pc0 being column lc0 of the WINDOW (>= 0).  The packed buffer holds
// one row of pitch_words u32 per storage row, row r0 first: bytes MSB first, window
// column j at bit 7 - (j & 7) of byte j >> 3.  A run whose last word
// (lc0 + ncols - 1) / 32 is not below pitch_words is hipErrorInvalidValue.
// get: the cells are OR-ed into `out` (the caller clears it; launches that share words
// are ordered on one stream), only words that hold cells of the run are written.
// put: exactly these cells change; storage columns >= active_cols are stored as 0;
// every other bit of `in` is ignored.
hipError_t launch_get_bits(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, uint32_t *out, int64_t out_pitch_words, int bit_gw, hipStream_t s);
hipError_t launch_put_bits(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, int64_t active_cols, const uint32_t *in, int64_t in_pitch_words, int bit_gw,
                           hipStream_t s);

// ---- gol_fill_random*: the counter-based random fill (gol_fill.h, gol_fill.hip) ----
// launch_put_bits's cells: storage rows [r0, r1) × storage columns [pc0, pc0 + ncols);
// storage row r0 is GLOBAL row grow0 and storage column pc0 is GLOBAL column lc0.
// Exactly these cells change: each takes X(r, c) < T of gol_fill.h with K = sm(seed)
// (T > 2^32 is hipErrorInvalidValue); storage columns >= active_cols are stored as 0.
hipError_t launch_fill_random(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                              int64_t lc0, int64_t ncols, int64_t active_cols, uint64_t K, uint64_t T, int bit_gw,
                              hipStream_t s);

// ---- gol_copy_window / gol_copy: board-to-board copies (gol_copy.h, gol_copy.hip) ----
// nrows storage rows from sr0 of `src` (pitch src_pitch_bytes, storage form src_gw) ×
// its storage columns [spc0, spc0 + ncols) are merged into the rows from dr0 of `dst`
// × its storage columns [dpc0, dpc0 + ncols) under op (GOL_COPY_*); *_gw: 0 = byte
// layout, else the bit layout's group width.  Exactly these cells of dst change;
// destination storage columns >= active_cols are stored as 0.  Of src only the units
// that hold cells of the run are read.  src and dst may be one buffer when the two
// rectangles are disjoint.  The two buffers live on the device of stream s.
hipError_t launch_copy_cells(const void *src, int64_t src_pitch_bytes, int64_t sr0, int64_t spc0, int src_gw, void *dst,
                             int64_t dst_pitch_bytes, int64_t dr0, int64_t dpc0, int dst_gw, int64_t nrows,
                             int64_t ncols, int64_t active_cols, int op, hipStream_t s);

// ---- gol_format_rle / gol_write_rle / gol_rle_bytes: RLE text of packed rows (gol_rle.h, gol_rle.hip) ----
// `packed` holds nrows rows of pitch_words u32 as launch_get_bits leaves them (pad bits 0), ncols >= 1
// cells each.  rows: tokens and token bytes (no newlines) per row.  scan (one workgroup): row r of the
// block is window row row_base + r; last_row = the last non-empty window row before the block (-1: none),
// tok0 = the tokens before it, L = tokens per line; per row the `$` count (0: none), the index of its
// first token and its byte offset in the block's text; *rec = the block's bytes, the token index and the
// last non-empty row behind it.  write: the tokens at their offsets (rec->bytes bytes of `text`).
struct RleRecord;
hipError_t launch_rle_rows(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols, uint32_t *ntok,
                           uint32_t *nraw, hipStream_t s);
hipError_t launch_rle_scan(const uint32_t *ntok, const uint32_t *nraw, int64_t nrows, int64_t row_base,
                           int64_t last_row, int64_t tok0, int L, uint32_t *dcount, int64_t *tix, int64_t *off,
                           RleRecord *rec, hipStream_t s);
hipError_t launch_rle_write(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols,
                            const uint32_t *ntok, const uint32_t *dcount, const int64_t *tix, const int64_t *off, int L,
                            char *text, hipStream_t s);

} // namespace gol
