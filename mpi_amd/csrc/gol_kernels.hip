// gol_kernels.hip — hand-written gfx950 (CDNA4) kernels for the Game-of-Life
// generation update (the reference's updateBoard/next, main.cpp:79-103 and
// main_serial.cpp:45-71) and its initialisation (initializeBoard,
// main.cpp:68-77 / main_serial.cpp:34-43).
//
// Design: every stencil kernel is a *register pipeline*.  One
// wave owns a column strip (64 lanes × V u32 words, lanes 0 and 63 are halo
// lanes that are computed but not stored) and walks down a chunk of rows.
// Each row is loaded from HBM exactly once per launch (coalesced V·4-byte
// vectors, prefetched 3 rows ahead) and each output row is stored once.  K
// generations are fused: stage g keeps a 3-row window of generation g-1 in
// VGPRs, so K generations cost one HBM read + one HBM write per cell.
// Horizontal neighbours within a lane come from v_alignbit funnel shifts, and
// across lanes from DPP wave_shr:1 / wave_shl:1 row moves (no LDS round trip).
//
//  * bit layout : 32 cells per word; a row's horizontal 3-sums are two bit-
//                 sliced planes (h0,h1); the vertical 9-sum and the B3/S23
//                 rule are 8 v_bitop3 ops per 32 cells.
//  * byte layout: 1 cell per byte in HBM.  Default: the bytebit kernel packs
//                 each loaded row into bit planes in registers, runs the bit
//                 pipeline (k up to 32, one wave per strip; k = 48 / 64 as a
//                 chain of waves per strip) and unpacks before the store;
//                 bytepair_chain_kernel runs the byte rows through the bit
//                 board's row-pair waves (GOL_OPT_BYTE_CORE = 4, k = 56); the
//                 SWAR kernel (v_add3_u32 sums of 4 cells per dword) serves
//                 k <= 8 when asked for.
//  * bit layout, k = 16 / 32: bit_chain_kernel, a chain of row-pair waves per
//                 strip handing rows through LDS (the headline at k = 16).
//  * bit layout, life-like rules other than B3/S23 (k <= 7): bit_rule_kernel, the
//                 bit pipeline with the table-driven stage of gol_rule.h (end of file).
//  * bit layout, the rules of GOL_COMPILED_RULES (k <= 7): bit_crule_kernel, the same
//                 pipeline with the rule as the stage's immediates (very end of file).
#include "gol_internal.h"
#include "gol_digest.h"
#include "gol_density.h"

#include <algorithm>
#include <cstdlib>
#include <utility>
#include <type_traits>
#include <cmath>
#include <map>
#include <mutex>

namespace gol {

// ------------------------------------------------------------- wave helpers

// lane i <- lane i-1 (lane 0 <- 0).  DPP wave_shr:1, a GFX9 full-wave row move.
__device__ __forceinline__ uint32_t from_left_lane(uint32_t x) {
    return __builtin_amdgcn_update_dpp(0u, x, 0x138, 0xf, 0xf, true);
}
// lane i <- lane i+1 (lane 63 <- 0).  DPP wave_shl:1.
__device__ __forceinline__ uint32_t from_right_lane(uint32_t x) {
    return __builtin_amdgcn_update_dpp(0u, x, 0x130, 0xf, 0xf, true);
}
// (hi:lo) >> s, low 32 bits — one v_alignbit_b32.
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t s) {
    return __builtin_amdgcn_alignbit(hi, lo, s);
}

// XCD-aware block remap: consecutive logical blocks land on one XCD (blocks are
// dealt round-robin over the 8 XCDs), so neighbouring strips/chunks share an L2.
// Bijective for any nblocks.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, x = b & 7, i = b >> 3;
    return (x < r) ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i;
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 3-input boolean ops as single v_bitop3_b32 (truth tables over a=0xF0, b=0xCC, c=0xAA).
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t maj(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}

// Raw buffer I/O.  The resource is wave-uniform; an offset >= num_records reads
// 0 / drops the store, so invalid rows and lanes need no branch and no select,
// and every load is issued unconditionally (exact vmcnt accounting: the
// compiler can keep the row prefetch in flight).
constexpr uint32_t kOOB = 0x40000000u;   // > any window's num_records

// AUX = cache-policy bits of the instruction (2: non-temporal, the streaming
// HBM-bound kernels; tools/hbm_probe.hip measures it).
template <int V, int AUX = 0>
__device__ __forceinline__ void buf_load(uint32_t (&d)[V], __amdgpu_buffer_rsrc_t r, uint32_t off) {
    if constexpr (V == 1) {
        d[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX);
    } else if constexpr (V == 2) {
        const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, AUX);
        d[0] = t.x; d[1] = t.y;
    } else {
        static_assert(V % 4 == 0, "V must be 1, 2 or a multiple of 4");
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r, off + 16 * q, 0, AUX);
            d[4 * q] = t.x; d[4 * q + 1] = t.y; d[4 * q + 2] = t.z; d[4 * q + 3] = t.w;
        }
    }
}
template <int V, int AUX = 0>
__device__ __forceinline__ void buf_store(__amdgpu_buffer_rsrc_t r, uint32_t off, const uint32_t (&s)[V]) {
    if constexpr (V == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(s[0], r, off, 0, AUX);
    } else if constexpr (V == 2) {
        u32x2 t; t.x = s[0]; t.y = s[1];
        __builtin_amdgcn_raw_buffer_store_b64(t, r, off, 0, AUX);
    } else {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            u32x4 t; t.x = s[4 * q]; t.y = s[4 * q + 1]; t.z = s[4 * q + 2]; t.w = s[4 * q + 3];
            __builtin_amdgcn_raw_buffer_store_b128(t, r, off + 16 * q, 0, AUX);
        }
    }
}

// Column strips of a row of T lane-units (a unit = the V words one lane holds).
// A strip is one wave of 64 lanes; a lane's horizontal neighbours come from the
// adjacent lanes, so an interior strip's lanes 0 and 63 are halo (computed, not
// stored) and it stores 62 units.  At the grid's left and right edges the
// neighbour outside is the dead boundary, which is what the lane move's zero
// fill supplies, so the first strip stores lanes 0..62 and the last strip
// (aligned to end at unit T-1) stores up to its lane 63: T units take
// 2 + ceil((T - 126) / 62) strips (131072 bit columns = 2048 units: 33).
__host__ __device__ inline int strip_count(int T) {
    return T <= 64 ? 1 : (T <= 126 ? 2 : 2 + (T - 126 + 61) / 62);
}
__host__ __device__ inline void strip_geometry(int T, int s, int &base, int &lo, int &hi) {
    const int ns = strip_count(T);
    if (ns == 1) {
        base = 0, lo = 0, hi = T;
    } else if (s == 0) {
        base = 0, lo = 0, hi = 63;
    } else if (s < ns - 1) {
        base = 62 * s, lo = 62 * s + 1, hi = 62 * s + 63;
    } else {
        base = T - 64, lo = 62 * (s - 1) + 63, hi = T;
    }
}
// Folded tail strip (the k = 8 pair kernel on 4-word groups).  Above, the last
// strip stores only the units left over past the interior strips: at 131072
// columns (T = 1024 units of 128 columns) 31 of its 64 lanes, so 17 strips do
// the work of 16.5.  When the leftover is at most 30 units, strips
// 0..ns-3 stay as above, strip ns-2 is aligned to end at unit T-1 (stores its
// lanes 1..63) and the gap of `fold_gap` units before it is covered by strip
// ns-1, the FOLDED strip: its two half-waves hold the same 32 units (a halo
// lane at each end of a half) for two different row ranges — lanes 32-63 read
// and write rows shifted by the first half's height — so one wave covers the
// gap for two chunk-rows.  Lanes 31 and 32 take each other's words through the
// lane moves: both are halo lanes, whose garbage (one column per generation)
// stays inside their 128 columns.  Returns 0 when the geometry does not fold.
__host__ __device__ inline int fold_gap(int T) {
    const int ns = strip_count(T);
    if (ns < 3) return 0;
    const int gap = T - 64 - 62 * (ns - 2);
    return (gap >= 1 && gap <= 30) ? gap : 0;
}
__host__ __device__ inline void strip_geometry_fold(int T, int s, int &base, int &lo, int &hi) {
    const int ns = strip_count(T);
    if (s < ns - 2) {
        strip_geometry(T, s, base, lo, hi);
    } else if (s == ns - 2) {
        base = T - 64, lo = T - 63, hi = T;
    } else {   // the folded strip (per half)
        base = 62 * (ns - 2), lo = base + 1, hi = lo + fold_gap(T);
    }
}

// Per-wave geometry shared by the bit and byte pipelines.  Everything that is
// the same for the whole wave is made provably uniform so it lives in SGPRs.
// Bit layout: groups of G = a.gw words, column c in word G·(c / 32G) + c % G,
// bit (c % 32G) / G (gol_internal.h bit_word / bit_pos); a lane holds whole groups.
template <int V>
struct Strip {
    uint32_t ld_off;     // lane byte offset for loads (kOOB if outside the row pitch)
    uint32_t st_off;     // lane byte offset for stores (kOOB for halo lanes / inactive words)
    uint32_t mask[V];    // active-cell mask per word
    int R0, R1;          // output rows of this wave's chunk (uniform)
    int base_row;        // first row of the buffer window = R0 - K (uniform)
    __amdgpu_buffer_rsrc_t src, dst;
    __amdgpu_buffer_rsrc_t dst_out;   // (pair kernel) dst over exactly the output rows [R0, R1)
    u32x4 src4;          // src as 4 descriptor dwords (the LDS-DMA asm takes an SGPR quad)

    // One work item: column strip `strip`, output rows [r0, r1).
    // full == 0: bit layout (masks from active_cols); otherwise the byte
    // layout's per-dword cell mask (0x01010101).
    __device__ __forceinline__ void setup(const StencilArgs &a, int K, int strip, int r0, int r1, uint32_t full) {
        const int lane = threadIdx.x & 63;
        int base, lo, hi;   // first lane-unit (V words) of the strip; units [lo, hi) are stored
        strip_geometry((a.nunits + V - 1) / V, strip, base, lo, hi);
        const int64_t unit = base + lane;
        setup_unit(a, K, unit, unit >= lo && unit < hi, r0, r1, full);
    }
    // The same for an explicit lane unit (the pair kernel: strip_geometry_fold).
    __device__ __forceinline__ void setup_unit(const StencilArgs &a, int K, int64_t unit, bool stored, int r0, int r1,
                                               uint32_t full) {
        const int G = a.gw;
        const int64_t word0 = unit * V;
        const bool lane_in = word0 + V <= a.pitch;
        ld_off = lane_in ? (uint32_t)(word0 * 4) : kOOB;
        st_off = stored ? (uint32_t)(word0 * 4) : kOOB;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t wi = word0 + j;
            if (full) {
                mask[j] = (wi >= a.nunits) ? 0u : (wi == a.nunits - 1 ? a.last_mask : full);
            } else {   // word wi holds columns 32G·(wi/G) + G·bit + wi%G (G: 2 or 4, a power of two)
                const int64_t c0 = (wi / G) * (32 * G) + (wi % G);
                const int64_t n = (a.active_cols - c0 + G - 1) / G;
                mask[j] = n <= 0 ? 0u : (n >= 32 ? 0xffffffffu : ((1u << n) - 1u));
            }
        }
        rows(a, K, r0, r1, r1);
    }
    // Output rows [r0, r1) walked; the source window spans [r0 - K, rend + K)
    // (dst the same window), dst_out exactly [r0, rend) (rend > r1: the folded
    // strip's second half-wave, whose rows past rend fall outside).
    __device__ __forceinline__ void rows(const StencilArgs &a, int K, int r0, int r1, int rend) {
        R0 = r0;
        R1 = r1;
        base_row = R0 - K;
        const int64_t pitch_b = a.pitch * 4;
        const int win_rows = rend - R0 + 2 * K;
        const int nrec = (int)(win_rows * pitch_b);
        const uint8_t *sb = static_cast<const uint8_t *>(a.src) + (int64_t)base_row * pitch_b;
        src = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(sb), 0, nrec, 0x00020000);
        const uint64_t sa = reinterpret_cast<uint64_t>(sb);
        src4.x = __builtin_amdgcn_readfirstlane((uint32_t)sa);
        src4.y = __builtin_amdgcn_readfirstlane((uint32_t)(sa >> 32) & 0xffffu);   // stride 0
        src4.z = (uint32_t)nrec;
        src4.w = 0x00020000u;
        dst = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)base_row * pitch_b, 0,
                                                nrec, 0x00020000);
        dst_out = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)R0 * pitch_b, 0,
                                                    (int)((rend - R0) * pitch_b), 0x00020000);
    }
    // as row_off, also kOOB for rr >= lim; computed unconditionally and selected
    // once (a branch here would split the unrolled loop body into basic blocks)
    __device__ __forceinline__ uint32_t row_off_lim(const StencilArgs &a, int rr, int lim) const {
        const uint32_t off = (uint32_t)((rr - base_row) * (int)(a.pitch * 4));
        return ((rr >= a.row_lo) & (rr < a.row_hi) & (rr < lim)) ? off : kOOB;
    }
    // byte offset of window row `rr` if it is a live row, else kOOB (uniform)
    __device__ __forceinline__ uint32_t row_off(const StencilArgs &a, int rr) const {
        return (rr >= a.row_lo && rr < a.row_hi) ? (uint32_t)((rr - base_row) * (int)(a.pitch * 4)) : kOOB;
    }
};

// Work items of a launch (static: wave w of the grid takes item w).
//  plain : `rows_per`-row chunks, band-major and strip-minor, so neighbouring
//          strips of one band run together and share an L2.
//  guided: XCD x (= physical block % 8) owns the row band
//          [x·rows/8, (x+1)·rows/8); its waves, in dispatch order, take
//          chunk-rows whose height shrinks round by round (cpr chunk-rows per
//          round, heights h[r]), so early waves amortise the 2k-row warm-up
//          over tall chunks and the launch ends on short ones.
//  fold  : (strip_geometry_fold) the chunk-rows of a band (plain: of the
//          launch) come in pairs: the nstrips-1 ordinary strips of each, then
//          ONE folded-strip item covering both chunk-rows.  The band's first and
//          last chunk-rows stay unpaired (every strip, the folded one over that
//          chunk-row only): a pair at the dead row boundary would run as one tall
//          two-chunk wave (the kernels' fallback) and end the launch late.
struct Sched {
    int nitems;
    int rows_per;
    int guided, cpr, nrounds;
    int h[8];
    int fold;
};

// Items of a band of C chunk-rows on ns strips with a folded strip.
__host__ __device__ inline int fold_items(int C, int ns) {
    return C <= 2 ? C * ns : 2 * ns + (C - 1) / 2 * (2 * ns - 1);
}

// (strip, chunk-row) of item j of a band of C chunk-rows; pair: the folded item
// of chunk-rows cr and cr + 1.  False: no such item.
__device__ __forceinline__ bool item_of(const Sched &q, int nstrips, int C, int j, int &strip, int &cr, bool &pair) {
    pair = false;
    if (!q.fold) {
        cr = j / nstrips;
        strip = j - cr * nstrips;
        return true;
    }
    if (j < nstrips || C <= 2) {   // chunk-row 0 (and 1 when C <= 2), unpaired
        cr = j / nstrips;
        strip = j - cr * nstrips;
        return cr < C;
    }
    j -= nstrips;
    const int nr = nstrips - 1, P = 2 * nr + 1, np = (C - 1) / 2;   // pairs over chunk-rows 1 .. C-2
    if (j >= np * P) {   // the last chunk-row, unpaired
        cr = C - 1;
        strip = j - np * P;
        return strip < nstrips;
    }
    const int p = j / P, k = j - p * P;
    pair = k == 2 * nr;
    const int second = (!pair && k >= nr) ? 1 : 0;
    cr = 1 + 2 * p + second;
    strip = pair ? nr : k - second * nr;
    if (cr > C - 2) return false;   // (C even: the last pair has one chunk-row)
    pair = pair && cr + 1 <= C - 2;
    return true;
}

// Chunk-rows of band x that hold rows (guided).
__device__ __forceinline__ int guided_count(const StencilArgs &a, const Sched &q, int x) {
    const int rows = a.out_r1 - a.out_r0;
    const int len = (int)((int64_t)(x + 1) * rows / 8) - (int)((int64_t)x * rows / 8);
    int row = 0, n = 0;
    for (int r = 0; r < q.nrounds; ++r) {
        const int span = q.cpr * q.h[r];
        if (row + span >= len) return n + (len - row + q.h[r] - 1) / q.h[r];
        row += span;
        n += q.cpr;
    }
    return n;
}

__device__ __forceinline__ bool guided_rows(const StencilArgs &a, const Sched &q, int x, int cr, int &r0, int &r1) {
    const int r = cr / q.cpr;
    if (r >= q.nrounds) return false;
    int row = 0;
    for (int i = 0; i < r; ++i) row += q.cpr * q.h[i];
    row += (cr - r * q.cpr) * q.h[r];
    const int rows = a.out_r1 - a.out_r0;
    const int bs = a.out_r0 + (int)((int64_t)x * rows / 8), be = a.out_r0 + (int)((int64_t)(x + 1) * rows / 8);
    r0 = bs + row;
    if (r0 >= be) return false;
    r1 = min(r0 + q.h[r], be);
    return true;
}

// Runs `body(strip, r0, r1, r2)` for this wave's item, if it has one
// (wave-uniform): output rows [r0, r1), and for a folded item the next
// chunk-row [r1, r2) too (r2 == r1 otherwise, or when there is none).
template <typename F>
__device__ __forceinline__ void for_each_item2(const StencilArgs &a, const Sched &q, int nstrips, int nblocks,
                                               F &&body) {
    int strip, cr, r0, r1, r2;
    bool pair;
    if (q.guided) {
        const int x = blockIdx.x & 7;
        const int j = __builtin_amdgcn_readfirstlane((blockIdx.x >> 3) * 4 + (threadIdx.x >> 6));
        if (!item_of(q, nstrips, q.fold ? guided_count(a, q, x) : 0, j, strip, cr, pair)) return;
        if (!guided_rows(a, q, x, cr, r0, r1)) return;
        int b0, b1;
        r2 = (pair && guided_rows(a, q, x, cr + 1, b0, b1)) ? b1 : r1;
    } else {
        const int w = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nblocks) * 4 + (threadIdx.x >> 6));
        if (w >= q.nitems) return;
        const int nb = (a.out_r1 - a.out_r0 + q.rows_per - 1) / q.rows_per;
        if (!item_of(q, nstrips, nb, w, strip, cr, pair)) return;
        r0 = a.out_r0 + cr * q.rows_per;
        if (r0 >= a.out_r1) return;
        r1 = min(r0 + q.rows_per, a.out_r1);
        r2 = pair ? min(r1 + q.rows_per, a.out_r1) : r1;
    }
    body(strip, r0, r1, r2);
}
template <typename F>
__device__ __forceinline__ void for_each_item(const StencilArgs &a, const Sched &q, int nstrips, int nblocks,
                                              F &&body) {
    for_each_item2(a, q, nstrips, nblocks, [&](int strip, int r0, int r1, int) { body(strip, r0, r1); });
}
// The same for a plain plan (no guided rounds, no folded strip), decoded with
// nothing but the item index: the short-chunk HBM-bound kernels (k = 1, 16-row
// items) spend a visible share of each wave in the general decoding's
// dependent argument loads.
template <typename F>
__device__ __forceinline__ void for_each_item_plain(const StencilArgs &a, const Sched &q, int nstrips, int nblocks,
                                                    F &&body) {
    const int w = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, nblocks) * 4 + (threadIdx.x >> 6));
    if (w >= q.nitems) return;
    const int cr = w / nstrips, strip = w - cr * nstrips;
    const int r0 = a.out_r0 + cr * q.rows_per;
    if (r0 >= a.out_r1) return;
    body(strip, r0, min(r0 + q.rows_per, a.out_r1));
}

// ---------------------------------------------------------------- bit layout

// Horizontal 3-sums of one row of cells as two bit planes, h0 = L ^ C ^ R and
// h1 = maj(L, C, R).  In a 2-word group a cell's left/right neighbours are the
// SAME bit of the other word, except at the group ends: there one funnel shift
// (v_alignbit) brings in the neighbouring group's end bit, from this lane or —
// for the lane's first/last group — from the adjacent lane (DPP wave_shr /
// wave_shl, no LDS).  Per lane-row: 2 DPP + 2·V/2 v_alignbit.
template <int V, int G = kGroupWords>
__device__ __forceinline__ void hsum(const uint32_t (&nv)[V], uint32_t (&h0)[V], uint32_t (&h1)[V]) {
    const uint32_t lft = from_left_lane(nv[V - 1]);
    const uint32_t rgt = from_right_lane(nv[0]);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        uint32_t L, R;
        if (j % G == 0) L = funnel(nv[j + G - 1], j == 0 ? lft : nv[j - 1], 31);   // column 64·grp - 1
        else L = nv[j - 1];
        if (j % G == G - 1) R = funnel(j == V - 1 ? rgt : nv[j + 1], nv[j - G + 1], 1);   // column 64·(grp+1)
        else R = nv[j + 1];
        h0[j] = xor3(L, nv[j], R);
        h1[j] = maj(L, nv[j], R);
    }
}

// B3/S23 on bit-sliced horizontal 3-sums of rows above (a), at (b), below (c):
// 9-sum incl. self = o + 2u + 4(q+v); next = (sum==3) | (alive & sum==4).
// 8 v_bitop3_b32.  `mask` = 0 forces the cell dead (columns outside the grid);
// with alive = 0 there, the result is 0.
__device__ __forceinline__ uint32_t life_bits(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                              uint32_t c0, uint32_t c1, uint32_t alive,
                                              uint32_t mask) {
    const uint32_t o = xor3(a0, b0, c0);
    const uint32_t co = maj(a0, b0, c0);
    const uint32_t p = xor3(a1, b1, c1);
    const uint32_t q = maj(a1, b1, c1);
    const uint32_t u = __builtin_amdgcn_bitop3_b32(co, p, mask, 0x28);   // (co ^ p) & mask
    const uint32_t s = __builtin_amdgcn_bitop3_b32(q, co, p, 0x78);      // q ^ (co & p)
    const uint32_t m = __builtin_amdgcn_bitop3_b32(u, o, s, 0x42);       // u ? o & ~s : ~o & s
    return __builtin_amdgcn_bitop3_b32(m, u, alive, 0xE0);              // m & (u | alive)
}
// The same without a column mask (every cell of the word is inside the grid):
// u is a two-input v_xor_b32, and the mask needs no register.
__device__ __forceinline__ uint32_t life_bits_full(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                   uint32_t c0, uint32_t c1, uint32_t alive) {
    const uint32_t o = xor3(a0, b0, c0);
    const uint32_t co = maj(a0, b0, c0);
    const uint32_t p = xor3(a1, b1, c1);
    const uint32_t q = maj(a1, b1, c1);
    const uint32_t u = co ^ p;
    const uint32_t s = __builtin_amdgcn_bitop3_b32(q, co, p, 0x78);      // q ^ (co & p)
    const uint32_t m = __builtin_amdgcn_bitop3_b32(u, o, s, 0x42);       // u ? o & ~s : ~o & s
    return __builtin_amdgcn_bitop3_b32(m, u, alive, 0xE0);              // m & (u | alive)
}

// The rule stage of the register pipeline below is a functor, apply<EDGE>(the
// life_bits arguments).  This one is B3/S23 as the tuned truth tables above: no
// state, so the instantiations that name it compile to what they did when the
// two calls stood in bit_phase.  (The others: RuleStage and ConstRuleStage, at the end of the file.)
struct LifeStage {
    template <bool EDGE>
    __device__ __forceinline__ uint32_t apply(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0,
                                              uint32_t c1, uint32_t alive, uint32_t mask) const {
        if constexpr (EDGE) return life_bits(a0, a1, b0, b1, c0, c1, alive, mask);
        else return life_bits_full(a0, a1, b0, b1, c0, c1, alive);
    }
};

// The K-stage register pipeline.  Stage g keeps a 3-row window of generation
// g (the horizontal sums h0/h1 and the alive plane c of each row) and emits
// generation g+1 one row behind its input.  The K stages form NC chains of CL
// stages; chain ch > 0 consumes the row chain ch-1 produced in the PREVIOUS
// iteration (held in pend[]), so the chains of one iteration are independent
// dependency chains (ILP for few waves per SIMD).  NC = 1 is the plain
// pipeline.  Cost of a chain boundary: V registers and one more warm-up row.
// The loop is unrolled by 6 phases: the windows rotate with period 3 and the
// load ring with period 6, so no loop-carried value is copied across the back
// edge (no forced wait on a just-issued prefetch).
// RING = load-ring slots, prefetch distance RING/2 rows (6: 3 ahead; 3: 2 ahead, 3·V fewer
// registers; 12: 6 ahead, more bytes in flight for the HBM-bound k).
template <int V, int K, int CL, int RING>
struct BitState {
    static constexpr int NC = (K + CL - 1) / CL;   // chains
    uint32_t h0[K][3][V], h1[K][3][V], c[K][3][V];
    uint32_t pend[NC][V];                          // output row of each chain (previous iteration)
    uint32_t ld[RING][V];
};

// EDGE: chunks near the dead row boundary or strips with cells outside the
// grid (per-row validity selects and column masks); otherwise neither.
template <int V, int K, int CL, int RING, int AUX, bool EDGE, int P, int G, typename ST = LifeStage>
__device__ __forceinline__ void bit_phase(BitState<V, K, CL, RING> &S, const Strip<V> &st, const StencilArgs &a,
                                          int it, int N, const ST &stage = ST{}) {
    constexpr int NC = BitState<V, K, CL, RING>::NC;
    constexpr int D = NC - 1;
    constexpr int PD = RING / 2;      // prefetch distance
    const int rho = st.R0 - K + it;   // generation-0 row arriving this iteration
    // prefetch row rho+PD (unconditional: OOB reads 0)
    // prefetch row rho+PD (unconditional: OOB reads 0).  The offset's select
    // compiles to a scalar branch that ends the phase's scheduling region; at
    // k=8 one region per phase is faster than one per unrolled loop trip.
    buf_load<V, AUX>(S.ld[(P + PD) % RING], st.src, st.ld_off + ((it + PD < N) ? st.row_off(a, rho + PD) : kOOB));
    constexpr int A = (P + 1) % 3, B = (P + 2) % 3, C = P % 3;
#pragma unroll
    for (int ch = NC - 1; ch >= 0; --ch) {   // descending: pend[ch-1] is read before chain ch-1 rewrites it
        uint32_t nv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) nv[j] = ch == 0 ? S.ld[P % RING][j] : S.pend[ch - 1][j];
#pragma unroll
        for (int g = ch * CL; g < (ch + 1) * CL && g < K; ++g) {
            // nv = generation g, row rho - g - ch: its horizontal sums into slot C
#define GOL_W(plane, g, slot, j) S.plane[g][slot][j]
            uint32_t n0[V], n1[V];
            hsum<V, G>(nv, n0, n1);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                GOL_W(h0, g, C, j) = n0[j];
                GOL_W(h1, g, C, j) = n1[j];
                GOL_W(c, g, C, j) = nv[j];
            }
            const int x = rho - g - ch - 1;   // generation g+1 row produced now
            const bool valid = !EDGE || (x >= a.row_lo && x < a.row_hi);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t o = stage.template apply<EDGE>(
                    GOL_W(h0, g, A, j), GOL_W(h1, g, A, j), GOL_W(h0, g, B, j), GOL_W(h1, g, B, j),
                    GOL_W(h0, g, C, j), GOL_W(h1, g, C, j), GOL_W(c, g, B, j), st.mask[j]);
                nv[j] = valid ? o : 0u;
            }
        }
        if (ch < NC - 1) {
#pragma unroll
            for (int j = 0; j < V; ++j) S.pend[ch][j] = nv[j];
        } else {   // generation K, row rho - K - D: stored when it lies in [R0, R1)  (it in [2K+D, N))
            const uint32_t roff = (it >= 2 * K + D && it < N)
                                      ? (uint32_t)((rho - K - D - st.base_row) * (int)(a.pitch * 4)) : kOOB;
            buf_store<V, AUX>(st.dst, st.st_off + roff, nv);
        }
    }
}

template <int V, int K, int CL, int RING, int AUX, bool EDGE, int G, typename ST, int... P>
__device__ __forceinline__ void bit_phases(BitState<V, K, CL, RING> &S, const Strip<V> &st, const StencilArgs &a,
                                           int it, int N, const ST &stage, std::integer_sequence<int, P...>) {
    (bit_phase<V, K, CL, RING, AUX, EDGE, P, G, ST>(S, st, a, it + P, N, stage), ...);
}

template <int V, int K, int CL, int RING, int AUX, bool EDGE, int G, typename ST = LifeStage>
__device__ __forceinline__ void bit_run(const Strip<V> &st, const StencilArgs &a, const ST &stage = ST{}) {
    using State = BitState<V, K, CL, RING>;
    State S;
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < V; ++j) GOL_W(h0, g, s, j) = GOL_W(h1, g, s, j) = GOL_W(c, g, s, j) = 0u;
#pragma unroll
    for (int c = 0; c < State::NC; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) S.pend[c][j] = 0u;
    const int N = (st.R1 - st.R0) + 2 * K + (State::NC - 1);
#pragma unroll
    for (int s = 0; s < RING / 2; ++s)
        buf_load<V, AUX>(S.ld[s], st.src, st.ld_off + (s < N ? st.row_off(a, st.R0 - K + s) : kOOB));
    // unrolled by lcm(3, RING) phases so every window and ring slot index is static
    constexpr int U = RING % 3 == 0 ? RING : 3 * RING;
    for (int it = 0; it < N; it += U)   // iterations past N are harmless: no loads, no stores
        bit_phases<V, K, CL, RING, AUX, EDGE, G, ST>(S, st, a, it, N, stage, std::make_integer_sequence<int, U>{});
}

// LDS row ring (the row-pair kernel below): generation-0 rows reach the
// pipeline through LDS instead of VGPRs.  ONE buffer_load_dwordx4 ... lds
// (LDS-DMA: lanes 0-31 fetch row A, lanes 32-63 row B, 16 B each) fills a
// 1-KiB slot with two rows, several events ahead, and a lane reads its 8 B of a
// row back with ds_read right before the first stage needs it.  The ring holds
// no VGPRs, and the loop waits on vmcnt only for a DMA issued several events
// earlier.  The compiler does not see asm loads, so every wait is explicit
// (s_waitcnt vmcnt(n) counted from the fixed VMEM sequence of an event).
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
template <int V> struct LdsVec;
template <> struct LdsVec<2> { typedef lds_u32x2 T; };
template <> struct LdsVec<4> { typedef lds_u32x4 T; };

__device__ __forceinline__ void dma_pair(const u32x4 &rsrc, uint32_t voff, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_addr), "s"(rsrc) : "memory");
}

struct LdsRing {
    uint32_t lds;        // LDS byte address of slot 0 (uniform, for M0)
    uint32_t dma_off;    // lane's byte offset in a row (PairRing), kOOB past the pitch
    bool hi;             // lane fetches row B of a pair
    uint32_t next = 0;   // bit_chain_kernel: LDS address of the next wave's ring (its input)
};

// ------------------------------------------------ bit layout, row-pair stages
// The 9-sum of output row x is H(x-1) + H(x) + H(x+1) (H = the horizontal
// 3-sum of a row, two bit planes).  Output rows r-1 and r share the pair sum
// P = H(r-1) + H(r) (0..6, binary p0/e0/e1), so a stage takes its input rows
// two at a time ("event") and per output row needs only P + H(r-2) (row r-1)
// or P + H(r+1) (row r): a 4-gate rule over (p0, e0, e1, a0, a1, alive)
// (tools/pair_search.c: exhaustive; no 3-gate circuit exists).  Per output
// word: 8 v_bitop3 (H 2, P 2, rule 4) against 10 for one row per stage; the
// lane moves per row are the same.  The rule relies on alive's row being
// inside the pair (alive ⇒ P ≥ 1, dead ⇒ P ≤ 5: the don't-cares the 4-gate
// circuit needs), which holds for both outputs.  An event's two input rows
// are one LDS ring slot (one LDS-DMA), 3 events ahead.
__device__ __forceinline__ uint32_t life_pair(uint32_t p0, uint32_t e0, uint32_t e1, uint32_t a0, uint32_t a1,
                                              uint32_t alive) {
    const uint32_t g1 = __builtin_amdgcn_bitop3_b32(p0, a0, alive, 0x43);
    const uint32_t g2 = __builtin_amdgcn_bitop3_b32(e0, e1, a1, 0x6d);
    const uint32_t g3 = __builtin_amdgcn_bitop3_b32(e0, a1, alive, 0x7d);
    return __builtin_amdgcn_bitop3_b32(g3, g1, g2, 0x18);
}

template <int K, int CL, int V = 2>
struct PairState {
    static constexpr int NC = (K + CL - 1) / CL;   // stage chains (as BitState)
    // per stage, two parity sets: H of rows r-2 (a) and r-1 (b), alive of r-1
    uint32_t a0[K][2][V], a1[K][2][V], b0[K][2][V], b1[K][2][V], bc[K][2][V];
    uint32_t pend[NC][2][V];   // each chain's 2 output rows of the previous event
};
// LDS ring slots (events) per wave: 3 events (6 rows) of prefetch (6 slots: 1 wave/SIMD,
// -6 %, profiles/r04p_slots6_ab.jsonl; 2 slots: -32 %, profiles/r02e_lds_ring_pair_ab.jsonl);
constexpr int kPairSlots = 4;
                                // even, so the state parity of every unrolled event is static
// LDS ring geometry per lane width V (words per lane): an event's two rows are
// V·512 B; V = 2: one DMA (lanes 0-31 row A, 32-63 row B, 16 B each), V = 4:
// one DMA per row (64 lanes × 16 B).  The lane offsets follow the ring.
template <int V>
struct PairRing {
    static constexpr int SLOT = 2 * 64 * 4 * V;           // bytes per event slot
    static constexpr int DMAS = V / 2;                     // DMAs per event
    static constexpr int OFFS = kPairSlots * SLOT;         // byte offset of the lane offsets
    static constexpr int WAVE = OFFS + 64 * 8;             // bytes per wave
    static constexpr int VMEM = DMAS + 2;                  // VMEM ops per event (DMAs + 2 stores)
    // a slot's last DMA was issued kPairSlots-1 events ago; after it: that event's
    // 2 stores and VMEM ops per event in between
    static constexpr int WAIT = 2 + (kPairSlots - 2) * VMEM;
    // a chain's first wave (bit_chain_kernel) hands its rows on through LDS: no stores
    static constexpr int WAIT_NOSTORE = (kPairSlots - 2) * DMAS;
};
// Words per lane V of the pair kernel = the group width G: the product runs
// V = G = 4 (one 128-column group per lane, 2 waves/SIMD).  The
// code also takes V = 2 (one 64-column group, 128 VGPRs, 4 waves/SIMD: rounds
// 2-3's kernel, 1.5-5.5 % slower) — not instantiated.

// Byte rows <-> 4-word bit groups (the byte board through the pair stages:
// bytepair_chain_kernel, pair_event IN = 2 / OUT = 2).
constexpr int kBPRow = 64 * 128;   // bytes of a strip row (64 lanes × 128 columns)

// 4×4 byte transpose: out[j] byte k = in[k] byte j (its own inverse)
__device__ __forceinline__ void bp_transpose(const uint32_t (&in)[4], uint32_t (&out)[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(in[1], in[0], 0x05010400u);   // in0.b0 in1.b0 in0.b1 in1.b1
    const uint32_t t1 = __builtin_amdgcn_perm(in[1], in[0], 0x07030602u);   // in0.b2 in1.b2 in0.b3 in1.b3
    const uint32_t t2 = __builtin_amdgcn_perm(in[3], in[2], 0x05010400u);
    const uint32_t t3 = __builtin_amdgcn_perm(in[3], in[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}
// 32 dwords of 0/1 bytes (x[i] = columns 4i .. 4i+3) -> 4 words (word j bit i =
// column 4i + j): e_k = OR x[8k+b] << b puts column 4(8k+b) + j at bit 8j + b
// of e_k, i.e. byte j of e_k is byte k of word j.
__device__ __forceinline__ void bp_pack(const uint32_t (&x)[32], uint32_t (&w)[4]) {
    uint32_t e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t t = x[8 * k];
#pragma unroll
        for (int b = 1; b < 8; ++b) t |= x[8 * k + b] << b;
        e[k] = t;
    }
    bp_transpose(e, w);
}
__device__ __forceinline__ void bp_unpack(const uint32_t (&w)[4], uint32_t (&x)[32]) {
    uint32_t e[4];
    bp_transpose(w, e);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 8; ++b) x[8 * k + b] = (e[k] >> b) & 0x01010101u;
}

// One event: generation-0 rows rho, rho+1 enter chain 0; stage g of chain ch
// takes generation-g rows r, r+1 (r = rho - g - 2ch) and emits generation
// g+1 rows r-1, r.  The last chain's rows are stored.
// PRO >= 0: the chunk's event PRO (< K), whose stages g > PRO only produce
// rows outside every stored row's light cone: they are skipped, and stage
// g == PRO only records its input rows' sums for the next event.  (Stage g's
// outputs of event ev are needed iff ev > g; its recorded sums iff ev >= g.)
// Chain roles (bit_chain_kernel): IN = 1 takes the event's rows from the ring
// slot the previous wave of the chain wrote (no DMA), OUT = 1 writes the two
// output rows into the next wave's ring slot E % kPairSlots instead of storing
// them, BAR = 1 ends the event with a workgroup barrier, BAR = 2 ends every
// second one (odd E) with it.  (0, 0, 0): the stand-alone kernel.
template <int K, int CL, bool EDGE, int E, int PRO = -1, int V = 2, int G = kGroupWords, int IN = 0, int OUT = 0,
          int BAR = 0>
__device__ __forceinline__ void pair_event(PairState<K, CL, V> &S, const Strip<V> &st, const StencilArgs &a,
                                           const LdsRing &L, int ev) {
    using R = PairRing<V>;
    using LV = typename LdsVec<V>::T;
    constexpr int NC = PairState<K, CL, V>::NC, D = NC - 1;
    constexpr int q = E & 1, slot = E % kPairSlots;
    const int rho = st.R0 - K + 2 * ev;
    // this slot's DMA(s) were issued kPairSlots-1 events ago (R::WAIT VMEM ops since)
    if constexpr (IN == 0)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OUT ? R::WAIT_NOSTORE : R::WAIT) : "memory");
    if constexpr (IN == 2)   // byte rows: 16 DMAs per event, no stores (OUT = 1)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kPairSlots - 2) * 16) : "memory");
    // The lane's ring address is recomputed every event (asm: not hoisted) and
    // its store / DMA offsets are re-read from LDS (after the ring), so none of
    // them holds a VGPR through the pipeline: K=8 fits 128 VGPRs (4 waves/SIMD).
    uint32_t lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const LV *rd = (const LV *)(uintptr_t)(L.lds + lane * (4 * V));
    uint32_t st_off, dma_off;
    if constexpr (IN == 2 || OUT == 2) {   // (the byte board's edge waves keep their offsets in VGPRs)
        st_off = st.st_off;
        dma_off = st.ld_off;
    } else {
        const u32x2 offs = *(volatile lds_u32x2 *)(uintptr_t)(L.lds + R::OFFS + lane * 8);
        st_off = offs.x;
        dma_off = offs.y;
    }
    // this event's rows, read together with the offsets (one LDS round trip at
    // the head of the event; the DMA below fills another slot: +1.6-7.7 % over
    // reading them after the DMA, profiles/r04n_fold_early_ab.jsonl)
    typename std::conditional<V == 4, u32x4, u32x2>::type ra, rb;
    if constexpr (IN == 2) {   // byte rows from the DMA ring slot (chunk q of the lane's 128 B at 1024·q + 16·lane)
        static_assert(V == 4, "byte rows feed 4-word groups");
        const lds_u32x4 *rbyte = (const lds_u32x4 *)(uintptr_t)(L.lds + slot * 2 * kBPRow + lane * 16);
        uint32_t xa[32], xb[32];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const u32x4 ta = rbyte[64 * c], tb = rbyte[kBPRow / 16 + 64 * c];
            xa[4 * c] = ta.x, xa[4 * c + 1] = ta.y, xa[4 * c + 2] = ta.z, xa[4 * c + 3] = ta.w;
            xb[4 * c] = tb.x, xb[4 * c + 1] = tb.y, xb[4 * c + 2] = tb.z, xb[4 * c + 3] = tb.w;
        }
        {   // rows of event ev + kPairSlots - 1 into the slot read at event ev - 1
            const int pr = rho + 2 * (kPairSlots - 1);
            const uint32_t oa = st.row_off_lim(a, pr, st.R1 + K), ob = st.row_off_lim(a, pr + 1, st.R1 + K);
            const uint32_t sl = L.lds + ((E + kPairSlots - 1) % kPairSlots) * 2 * kBPRow;
#pragma unroll
            for (int c = 0; c < 8; ++c) dma_pair(st.src4, dma_off + 16 * c + oa, sl + 1024 * c);
#pragma unroll
            for (int c = 0; c < 8; ++c) dma_pair(st.src4, dma_off + 16 * c + ob, sl + kBPRow + 1024 * c);
        }
        uint32_t wa[4], wb[4];
        bp_pack(xa, wa);
        bp_pack(xb, wb);
        ra.x = wa[0], ra.y = wa[1], ra.z = wa[2], ra.w = wa[3];
        rb.x = wb[0], rb.y = wb[1], rb.z = wb[2], rb.w = wb[3];
    } else {
        ra = rd[slot * 128];
        rb = rd[slot * 128 + 64];
    }
    if constexpr (IN == 0) {
        const int pr = rho + 2 * (kPairSlots - 1);
        const uint32_t oa = st.row_off_lim(a, pr, st.R1 + K), ob = st.row_off_lim(a, pr + 1, st.R1 + K);
        const uint32_t sl = L.lds + ((E + kPairSlots - 1) % kPairSlots) * R::SLOT;
        if constexpr (V == 2) {
            dma_pair(st.src4, dma_off + (L.hi ? ob : oa), sl);
        } else {
            dma_pair(st.src4, dma_off + oa, sl);
            dma_pair(st.src4, dma_off + ob, sl + R::SLOT / 2);
        }
    }
    // chain inputs: the new rows for chain 0, the previous event's rows of chain ch-1 for chain ch
    uint32_t x0[NC][V], x1[NC][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        x0[0][j] = ra[j];
        x1[0][j] = rb[j];
    }
#pragma unroll
    for (int ch = 1; ch < NC; ++ch)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            x0[ch][j] = S.pend[ch - 1][0][j];
            x1[ch][j] = S.pend[ch - 1][1][j];
        }
    // stage i of every chain in one scheduling region (the chains are independent:
    // ILP).  V = 4: one region per event (+0.6 % over one per stage, per 2 or 4
    // stages within 1 %, profiles/r04g_g4_variants_ab.jsonl, r04r_sb_ab.jsonl);
    // V = 2: one per stage index (keeps the register peak within 128 VGPRs)
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        if (V == 2 || i == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const int g = ch * CL + i;
            if (g >= K) continue;
            if (PRO >= 0 && NC == 1 && g > PRO) continue;
            constexpr bool sums_only_possible = PRO >= 0 && NC == 1;
            uint32_t X0[V], X1[V], Y0[V], Y1[V];
            hsum<V, G>(x0[ch], X0, X1);
            hsum<V, G>(x1[ch], Y0, Y1);
            const int r = rho - g - 2 * ch;
            const bool v0 = !EDGE || (r - 1 >= a.row_lo && r - 1 < a.row_hi);
            const bool v1 = !EDGE || (r >= a.row_lo && r < a.row_hi);
            if (sums_only_possible && g == PRO) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    S.a0[g][q ^ 1][j] = X0[j];
                    S.a1[g][q ^ 1][j] = X1[j];
                    S.b0[g][q ^ 1][j] = Y0[j];
                    S.b1[g][q ^ 1][j] = Y1[j];
                    S.bc[g][q ^ 1][j] = x1[ch][j];
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t B0 = S.b0[g][q][j], B1 = S.b1[g][q][j];
                const uint32_t p0 = B0 ^ X0[j], k = B0 & X0[j];
                const uint32_t e0 = xor3(B1, X1[j], k), e1 = maj(B1, X1[j], k);
                uint32_t o0 = life_pair(p0, e0, e1, S.a0[g][q][j], S.a1[g][q][j], S.bc[g][q][j]);
                uint32_t o1 = life_pair(p0, e0, e1, Y0[j], Y1[j], x0[ch][j]);
                if constexpr (EDGE) {
                    o0 = v0 ? (o0 & st.mask[j]) : 0u;
                    o1 = v1 ? (o1 & st.mask[j]) : 0u;
                }
                S.a0[g][q ^ 1][j] = X0[j];
                S.a1[g][q ^ 1][j] = X1[j];
                S.b0[g][q ^ 1][j] = Y0[j];
                S.b1[g][q ^ 1][j] = Y1[j];
                S.bc[g][q ^ 1][j] = x1[ch][j];
                x0[ch][j] = o0;
                x1[ch][j] = o1;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < NC - 1; ++ch)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            S.pend[ch][0][j] = x0[ch][j];
            S.pend[ch][1][j] = x1[ch][j];
        }
    {   // generation K, rows s, s+1 (s = rho - K - 2D): stored when in [R0, R1)
        const int s = rho - K - 2 * D;
        const int pb = (int)(a.pitch * 4);
        // dst_out spans the item's output rows (the folded strip: both chunk-rows;
        // its second half-wave's lane offsets add the first half's height, so
        // that half's rows past the item's end fall outside)
        const uint32_t f0 = (uint32_t)((s - st.R0) * pb), f1 = f0 + (uint32_t)pb;
        const uint32_t o0 = ((s >= st.R0) & (s < st.R1)) ? f0 : kOOB;
        const uint32_t o1 = ((s + 1 >= st.R0) & (s + 1 < st.R1)) ? f1 : kOOB;
        if constexpr (OUT == 0) {
            buf_store<V>(st.dst_out, st_off + o0, x0[NC - 1]);   // exactly two VMEM ops per event
            buf_store<V>(st.dst_out, st_off + o1, x1[NC - 1]);
        } else if constexpr (OUT == 2) {   // byte rows: unpacked, 8 × 16 B per row
            static_assert(V == 4, "byte rows from 4-word groups");
            uint32_t xx[32];
            bp_unpack(x0[NC - 1], xx);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t t[4] = {xx[4 * c], xx[4 * c + 1], xx[4 * c + 2], xx[4 * c + 3]};
                buf_store<4>(st.dst_out, st_off + o0 + 16 * c, t);
            }
            bp_unpack(x1[NC - 1], xx);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t t[4] = {xx[4 * c], xx[4 * c + 1], xx[4 * c + 2], xx[4 * c + 3]};
                buf_store<4>(st.dst_out, st_off + o1 + 16 * c, t);
            }
        } else {   // rows s, s+1 of generation K -> the next wave's slot E % kPairSlots (its event E input)
            (void)o0;
            (void)o1;
            LV *wr = (LV *)(uintptr_t)(L.next + slot * R::SLOT + lane * (4 * V));
            typename std::conditional<V == 4, u32x4, u32x2>::type va, vb;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                va[j] = x0[NC - 1][j];
                vb[j] = x1[NC - 1][j];
            }
            wr[0] = va;
            wr[64] = vb;
        }
    }
    if constexpr (BAR == 1 || (BAR == 2 && (E & 1))) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int K, int CL, bool EDGE, int V, int G, int... E>
__device__ __forceinline__ void pair_events(PairState<K, CL, V> &S, const Strip<V> &st, const StencilArgs &a,
                                            const LdsRing &L, int ev, int NE, std::integer_sequence<int, E...>) {
    // (a branch around each event of the last trip made the register allocator
    // spill across the whole loop: the trip runs whole; events past NE store nothing)
    (void)NE;
    (pair_event<K, CL, EDGE, E, -1, V, G>(S, st, a, L, ev + E), ...);
}

template <int K, int CL, bool EDGE, int V, int G, int... E>
__device__ __forceinline__ void pair_prologue(PairState<K, CL, V> &S, const Strip<V> &st, const StencilArgs &a,
                                              const LdsRing &L, std::integer_sequence<int, E...>) {
    (pair_event<K, CL, EDGE, E % kPairSlots, E, V, G>(S, st, a, L, E), ...);
}

template <int K, int CL, bool EDGE, int V, int G>
__device__ __forceinline__ void bit_run_pair(const Strip<V> &st, const StencilArgs &a, const LdsRing &L) {
    using State = PairState<K, CL, V>;
    constexpr int D = State::NC - 1;
    State S;
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < V; ++j)
                S.a0[g][p][j] = S.a1[g][p][j] = S.b0[g][p][j] = S.b1[g][p][j] = S.bc[g][p][j] = 0u;
#pragma unroll
    for (int c = 0; c < State::NC; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) S.pend[c][0][j] = S.pend[c][1][j] = 0u;
    // event ev stores generation-K rows R0-2K-2D+2ev and the next one: the last
    // event is the one that stores row R1-1
    const int NE = (st.R1 - 1 - st.R0 + 2 * K + 2 * D) / 2 + 1;
#pragma unroll
    for (int e = 0; e < kPairSlots - 1; ++e) {
        const int pr = st.R0 - K + 2 * e;
        const uint32_t oa = st.row_off(a, pr), ob = st.row_off(a, pr + 1);
        if constexpr (V == 2) {
            dma_pair(st.src4, L.dma_off + (L.hi ? ob : oa), L.lds + e * PairRing<V>::SLOT);
        } else {
            dma_pair(st.src4, L.dma_off + oa, L.lds + e * PairRing<V>::SLOT);
            dma_pair(st.src4, L.dma_off + ob, L.lds + e * PairRing<V>::SLOT + PairRing<V>::SLOT / 2);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ev0 = 0;
    if constexpr (State::NC == 1 && K % kPairSlots == 0) {   // events 0..K-1: NE > K always
        pair_prologue<K, CL, EDGE, V, G>(S, st, a, L, std::make_integer_sequence<int, K>{});
        ev0 = K;
    }
    for (int ev = ev0; ev < NE; ev += kPairSlots)   // events past NE are harmless: no stores inside [R0, R1)
        pair_events<K, CL, EDGE, V, G>(S, st, a, L, ev, NE, std::make_integer_sequence<int, kPairSlots>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA into LDS outlives the wave
}

template <int K, int NCH, int V = 2, int G = kGroupWords>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8 / V)))
void bit_pair_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    using R = PairRing<V>;
    __shared__ __attribute__((aligned(16))) uint8_t ring[4][R::WAVE];   // + lane offsets
    for_each_item2(a, q, nstrips, nblocks, [&](int strip, int r0, int r1, int r2) {
        constexpr int CL = (K + NCH - 1) / NCH;
        constexpr int M = 2 * K + 2 * ((K - 1) / CL) + 2;
        const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int lane = threadIdx.x & 63;
        const int T = (a.nunits + V - 1) / V;
        const int64_t pb = a.pitch * 4;
        LdsRing L;
        L.lds = (uint32_t)(uintptr_t)&ring[w][0];
        L.hi = lane >= 32;
        // The folded strip (V = 4, strip_geometry_fold): lane l holds unit
        // base + l % 32 in both half-waves, lanes 0-31 on output rows [r0, r1),
        // lanes 32-63 on [r1, r2).  With the whole cone of [r0, r2) live and every
        // column inside the grid both halves run in ONE pass: the pipeline walks
        // [r0, r0 + h) (h = r1 - r0 >= r2 - r1), the second half's DMA and store
        // offsets carry + h rows, the source window spans [r0 - K, r2 + K) (rows
        // past it read 0 and reach only rows >= r2) and dst_out spans exactly
        // [r0, r2).  Otherwise (dead-boundary rows) lanes 0-31 walk [r0, r2) as one
        // tall chunk and lanes 32-63 recompute their columns and store nothing.
        const bool fs = V == 4 && q.fold && strip == nstrips - 1;
        int b, lo, hi;
        if (q.fold) strip_geometry_fold(T, strip, b, lo, hi);
        else strip_geometry(T, strip, b, lo, hi);
        const int64_t unit = b + (fs ? (lane & 31) : lane);
        bool stored = unit >= lo && unit < hi;
        Strip<V> st;
        st.setup_unit(a, K, unit, stored, r0, r1, 0u);
        uint32_t all = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < V; ++j) all &= st.mask[j];
        const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
        const int rend = fs ? r2 : r1;
        const bool edge = !(full && r0 - M >= a.row_lo && rend + M <= a.row_hi);
        // V = 2: lanes 0-31 / 32-63 each fetch 512 B of row A / B; V = 4: 16 B per lane per row
        const int64_t ubyte = V == 2 ? ((int64_t)b + 2 * (lane & 31)) * 8 : unit * 16;
        const uint32_t dma = (ubyte + 16 <= pb) ? (uint32_t)ubyte : kOOB;
        uint32_t dB = 0u;
        if (fs && !edge) {
            dB = lane >= 32 ? (uint32_t)((r1 - r0) * pb) : 0u;
            st.rows(a, K, r0, r1, r2);
        } else if (fs) {
            stored = stored && lane < 32;
            st.rows(a, K, r0, r2, r2);
        }
        u32x2 o;
        o.x = stored ? (uint32_t)(unit * (4 * V)) + dB : kOOB;   // the lane's words in a row
        o.y = dma == kOOB ? kOOB : dma + dB;
        L.dma_off = o.y;
        *(lds_u32x2 *)(uintptr_t)(L.lds + R::OFFS + lane * 8) = o;
        if (edge) bit_run_pair<K, CL, true, V, G>(st, a, L);
        else bit_run_pair<K, CL, false, V, G>(st, a, L);
    });
}

// ------------------------------------------ bit layout, chain of pair waves
// bit_chain_kernel<S, KW>: K = KW·S generations per HBM pass on the k = 8 layout
// (4-word groups).  A chain of S waves shares one (strip, chunk) item; wave s
// is the stand-alone row-pair pipeline of KW stages (bit_pair_kernel) for the
// output rows [R0 - KW(S-1-s), R1 + KW(S-1-s)) of generation KW(s+1): wave 0
// takes its rows from HBM through its LDS-DMA ring, wave s > 0 from its ring
// slots, which wave s-1 writes with its output rows (instead of storing them);
// the last wave stores.  Wave s starts chain_lag·s events late (its first
// input rows are wave s-1's event-KW output): the writer's event E + KW and the
// reader's event E use the same slot E % kPairSlots two events apart, and a
// workgroup barrier ends every second event, so a slot is written and read in
// consecutive barrier intervals and rewritten two intervals later.  Why: the board crosses HBM once
// per K generations instead of once per 8 — the k = 8 kernel at the same VALU
// work but no HBM traffic runs at +12 % clock on this power-limited chip
// (profiles/r06h_nohbm_probe.jsonl) — for the price of the hand-off through LDS
// (2 KiB written and read per event and wave boundary) and a barrier per event.
// 4 / S chains per 256-thread workgroup; all run the same number of barriers.
// KW = 8 (two waves at k = 16, four at k = 32) is what ships: k = 16 as four
// 4-stage waves (<4, 4, 3>: 148 VGPRs, no spill, 3 waves/SIMD) is parity-green
// but 6 % slower (profiles/r06p_chain4x4_ab.jsonl: 12 + 8 + 4 extra rows of
// halo stages per item and three hand-offs instead of one).
// events between consecutive waves of a chain of KW-stage waves: KW + one barrier
// interval (KW ≡ 0 mod 4 keeps the slot of every unrolled event static)
template <int KW>
constexpr int chain_lag() { return KW + 2; }
// (one stage chain of K stages per wave: CL = K)
template <int K, bool EDGE, int IN, int OUT, int... E>
__device__ __forceinline__ void chain_prologue(PairState<K, K, 4> &S, const Strip<4> &st, const StencilArgs &a,
                                               const LdsRing &L, std::integer_sequence<int, E...>) {
    (pair_event<K, K, EDGE, E % kPairSlots, E, 4, 4, IN, OUT, 2>(S, st, a, L, E), ...);
}
template <int K, bool EDGE, int IN, int OUT, int... E>
__device__ __forceinline__ void chain_events(PairState<K, K, 4> &S, const Strip<4> &st, const StencilArgs &a,
                                             const LdsRing &L, int ev, std::integer_sequence<int, E...>) {
    (pair_event<K, K, EDGE, E, -1, 4, 4, IN, OUT, 2>(S, st, a, L, ev + E), ...);
}

// events of a wave's stand-alone pipeline over output rows [R0, R1): the
// prologue's K plus whole trips of kPairSlots covering (R1 - R0 + 2K - 1) / 2 + 1
__device__ __forceinline__ int chain_wave_events(int rows, int K) {
    const int NE = (rows - 1 + 2 * K) / 2 + 1;
    return K + (NE - K + kPairSlots - 1) / kPairSlots * kPairSlots;
}

// One wave of a chain (KW pair stages): `pre` barriers, its pipeline (a barrier
// per two events; its event count is even), then barriers up to `total`.
template <int KW, bool EDGE, int IN, int OUT>
__device__ __forceinline__ void chain_wave(const Strip<4> &st, const StencilArgs &a, const LdsRing &L, int pre,
                                           int total) {
    constexpr int K = KW;
    using State = PairState<K, K, 4>;
    State S;
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                S.a0[g][p][j] = S.a1[g][p][j] = S.b0[g][p][j] = S.b1[g][p][j] = S.bc[g][p][j] = 0u;
    int done = 0;
    for (; done < pre; ++done) asm volatile("s_barrier" ::: "memory");
    if constexpr (IN == 0) {
#pragma unroll
        for (int e = 0; e < kPairSlots - 1; ++e) {
            const int pr = st.R0 - K + 2 * e;
            const uint32_t oa = st.row_off(a, pr), ob = st.row_off(a, pr + 1);
            dma_pair(st.src4, L.dma_off + oa, L.lds + e * PairRing<4>::SLOT);
            dma_pair(st.src4, L.dma_off + ob, L.lds + e * PairRing<4>::SLOT + PairRing<4>::SLOT / 2);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if constexpr (IN == 2) {   // byte rows (bytepair_chain_kernel's first wave)
#pragma unroll
        for (int e = 0; e < kPairSlots - 1; ++e)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t o = st.row_off(a, st.R0 - K + 2 * e + r);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    dma_pair(st.src4, st.ld_off + 16 * c + o, L.lds + e * 2 * kBPRow + r * kBPRow + 1024 * c);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const int NE = chain_wave_events(st.R1 - st.R0, K);
    chain_prologue<K, EDGE, IN, OUT>(S, st, a, L, std::make_integer_sequence<int, K>{});
    for (int ev = K; ev < NE; ev += kPairSlots)
        chain_events<K, EDGE, IN, OUT>(S, st, a, L, ev, std::make_integer_sequence<int, kPairSlots>{});
    done += NE / 2;
    for (; done < total; ++done) asm volatile("s_barrier" ::: "memory");
    if constexpr (IN != 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA into LDS outlives the wave
}

// (strip, r0, r1, r2) of item w (plain schedule, with the folded strip); false: none
__device__ __forceinline__ bool chain_item(const StencilArgs &a, const Sched &q, int nstrips, int w, int &strip,
                                           int &r0, int &r1, int &r2) {
    if (w >= q.nitems) return false;
    const int nb = (a.out_r1 - a.out_r0 + q.rows_per - 1) / q.rows_per;
    int cr;
    bool pair;
    if (!item_of(q, nstrips, nb, w, strip, cr, pair)) return false;
    r0 = a.out_r0 + cr * q.rows_per;
    if (r0 >= a.out_r1) return false;
    r1 = min(r0 + q.rows_per, a.out_r1);
    r2 = pair ? min(r1 + q.rows_per, a.out_r1) : r1;
    return true;
}

template <int S, int KW = 8, int WPE = 2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE)))
void bit_chain_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    constexpr int V = 4, K = KW * S, CPB = 4 / S, LAG = chain_lag<KW>();   // (CPB: chains per workgroup)
    using R = PairRing<V>;
    __shared__ __attribute__((aligned(16))) uint8_t ring[4][R::WAVE];   // + lane offsets
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = w % S, chain = w / S;
    const int lane = threadIdx.x & 63;
    const int T = (a.nunits + V - 1) / V;
    const int64_t pb = a.pitch * 4;
    // the barrier count of the workgroup: the largest of its chains' (wave S-1: LAG(S-1) idle
    // events before its pipeline, which is the longest)
    int strip = 0, r0 = 0, r1 = 0, r2 = 0, total = 0;
    bool mine = false;
#pragma unroll
    for (int c = 0; c < CPB; ++c) {
        int st_, a0, a1, a2;
        if (chain_item(a, q, nstrips, xcd_remap(blockIdx.x, nblocks) * CPB + c, st_, a0, a1, a2)) {
            // wave s runs LAG·s idle events, then its pipeline over h + 2KW(S-1-s)
            // rows (h = a1 - a0, or a2 - a0 for a folded item walked as one tall chunk):
            // 8 events per 16 rows, so the last wave's LAG(S-1) + NE(h) events are
            // the most; a2 - a0 >= either h; one barrier per two events
            total = max(total, (LAG * (S - 1) + chain_wave_events(a2 - a0, KW)) / 2);
            if (c == chain) {
                mine = true;
                strip = st_, r0 = a0, r1 = a1, r2 = a2;
            }
        }
    }
    if (total == 0) return;   // (no chain of this workgroup has an item)
    if (!mine) {              // the other chain's barriers
        for (int i = 0; i < total; ++i) asm volatile("s_barrier" ::: "memory");
        return;
    }
    LdsRing L;
    L.lds = (uint32_t)(uintptr_t)&ring[w][0];
    L.next = (uint32_t)(uintptr_t)&ring[s < S - 1 ? w + 1 : w][0];
    L.hi = lane >= 32;
    const bool fs = q.fold && strip == nstrips - 1;
    int b, lo, hi;
    if (q.fold) strip_geometry_fold(T, strip, b, lo, hi);
    else strip_geometry(T, strip, b, lo, hi);
    const int64_t unit = b + (fs ? (lane & 31) : lane);
    bool stored = unit >= lo && unit < hi;
    // wave s runs generations KW·s+1 .. KW·(s+1) on rows extended by KW per later wave
    const int ext = KW * (S - 1 - s);
    Strip<V> st;
    st.setup_unit(a, KW, unit, stored, r0 - ext, r1 + ext, 0u);
    uint32_t all = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < V; ++j) all &= st.mask[j];
    const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
    const int rend = fs ? r2 : r1;
    constexpr int M = 2 * K + 2;
    const bool edge = !(full && r0 - M >= a.row_lo && rend + M <= a.row_hi);
    const int64_t ubyte = unit * 16;
    const uint32_t dma = (ubyte + 16 <= pb) ? (uint32_t)ubyte : kOOB;
    uint32_t dB = 0u;
    // the folded strip: both half-waves in one pass (rows [r0, r0 + h) and, for lanes
    // 32-63, + h), or, near the dead row boundary, lanes 0-31 walk [r0, r2) alone
    if (fs && !edge) {
        dB = lane >= 32 ? (uint32_t)((r1 - r0) * pb) : 0u;
        st.rows(a, KW, r0 - ext, r1 + ext, r2 + ext);
    } else if (fs) {
        stored = stored && lane < 32;
        st.rows(a, KW, r0 - ext, r2 + ext, r2 + ext);
    }
    u32x2 o;
    o.x = (stored && s == S - 1) ? (uint32_t)(unit * (4 * V)) + dB : kOOB;   // the lane's words in a row
    o.y = dma == kOOB ? kOOB : dma + dB;
    L.dma_off = o.y;
    *(lds_u32x2 *)(uintptr_t)(L.lds + R::OFFS + lane * 8) = o;
    const int pre = LAG * s / 2;   // (barriers)
    if (s == 0) {
        if (edge) chain_wave<KW, true, 0, 1>(st, a, L, pre, total);
        else chain_wave<KW, false, 0, 1>(st, a, L, pre, total);
    } else if (s == S - 1) {
        if (edge) chain_wave<KW, true, 1, 0>(st, a, L, pre, total);
        else chain_wave<KW, false, 1, 0>(st, a, L, pre, total);
    } else {
        if constexpr (S > 2) {
            if (edge) chain_wave<KW, true, 1, 1>(st, a, L, pre, total);
            else chain_wave<KW, false, 1, 1>(st, a, L, pre, total);
        }
    }
}

// ------------------------------------------- byte board, chain of pair waves
// bytepair_chain_kernel<S>: K = 8·S generations per HBM pass on the BYTE board
// (1 B per cell in HBM, each cell read and written once per pass) through the
// bit board's row-pair stages — 9.1 VALU per word-update, where the byte
// board's one-word stages (bytebit_*) need 18.3.  A workgroup of S + 2 waves
// owns one (strip, chunk) item of 128-column lane units (bit_chain_kernel's
// strips, the folded tail strip included):
//   wave 0 (pack)    streams the item's byte rows through an LDS-DMA ring
//                    (16-B chunk q of lane l's 128 bytes at 1024·q + 16·l),
//                    packs each row into the 4-word group layout (word j bit i
//                    = column 4i + j of the lane's 128) and writes it into pair
//                    wave 0's ring slot, as a pair wave with OUT = 1 would;
//   waves 1 .. S     bit_chain_kernel's pair waves, all IN = 1, OUT = 1;
//   wave S + 1       (unpack) takes the last pair wave's rows from its slot,
//                    unpacks them to bytes and stores them.
// Pack and unpack cost 36 and 72 VALU per 128-column row, a pair wave ≈290.
// Pair wave 0 starts kBPLagIn events after the pack wave (its slot is written
// one barrier interval before it is read), every later wave chain_lag events
// after its writer; every wave ends each odd event with a workgroup barrier.
constexpr int kBPLagIn = 2;
// The pack wave: event E reads rows rho, rho+1 (rho = r0 - K + 2·ev) from its
// DMA ring slot E, refills the slot read at event E-1 with the rows of event
// ev + 3, and writes the packed rows into pair wave 0's slot E.
struct BPPack {
    uint32_t ld[8];   // the lane's 16-B chunk offsets in a row (kOOB past the pitch; + the fold shift)
    u32x4 src4;       // the window [r0 - K, rend + K)
    int base, lim;    // first window row, end of the window
    uint32_t bring, out;
};
template <int E>
__device__ __forceinline__ void bp_pack_event(const BPPack &P, const StencilArgs &a, int ev) {
    constexpr int DMAS = 16;   // per event: 2 rows × 8 chunks
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kPairSlots - 2) * DMAS) : "memory");
    const int lane = threadIdx.x & 63;
    const lds_u32x4 *rd = (const lds_u32x4 *)(uintptr_t)(P.bring + E * 2 * kBPRow + 16 * lane);
    uint32_t xa[32], xb[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const u32x4 ta = rd[64 * q], tb = rd[kBPRow / 16 + 64 * q];
        xa[4 * q] = ta.x, xa[4 * q + 1] = ta.y, xa[4 * q + 2] = ta.z, xa[4 * q + 3] = ta.w;
        xb[4 * q] = tb.x, xb[4 * q + 1] = tb.y, xb[4 * q + 2] = tb.z, xb[4 * q + 3] = tb.w;
    }
    {
        const int rr = P.base + 2 * (ev + kPairSlots - 1);
        const int64_t pb = a.pitch * 4;
        const uint32_t oa = (rr >= a.row_lo && rr < a.row_hi && rr < P.lim) ? (uint32_t)((rr - P.base) * pb) : kOOB;
        const uint32_t ob = (rr + 1 >= a.row_lo && rr + 1 < a.row_hi && rr + 1 < P.lim)
                                ? (uint32_t)((rr + 1 - P.base) * pb) : kOOB;
        const uint32_t sl = P.bring + ((E + kPairSlots - 1) % kPairSlots) * 2 * kBPRow;
#pragma unroll
        for (int q = 0; q < 8; ++q) dma_pair(P.src4, P.ld[q] + oa, sl + 1024 * q);
#pragma unroll
        for (int q = 0; q < 8; ++q) dma_pair(P.src4, P.ld[q] + ob, sl + kBPRow + 1024 * q);
    }
    uint32_t wa[4], wb[4];
    bp_pack(xa, wa);
    bp_pack(xb, wb);
    lds_u32x4 *wr = (lds_u32x4 *)(uintptr_t)(P.out + E * PairRing<4>::SLOT + 16 * lane);
    u32x4 va, vb;
    va.x = wa[0], va.y = wa[1], va.z = wa[2], va.w = wa[3];
    vb.x = wb[0], vb.y = wb[1], vb.z = wb[2], vb.w = wb[3];
    wr[0] = va;
    wr[64] = vb;
    if constexpr (E & 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
template <int... E>
__device__ __forceinline__ void bp_pack_trip(const BPPack &P, const StencilArgs &a, int ev,
                                             std::integer_sequence<int, E...>) {
    (bp_pack_event<E>(P, a, ev + E), ...);
}

// The unpack wave: event E takes rows r0 + 2·ev, r0 + 2·ev + 1 (generation K)
// from its ring slot E and stores the ones in [r0, R1).
struct BPUnpack {
    uint32_t st[8];   // the lane's 16-B chunk offsets in a row (kOOB: not stored; + the fold shift)
    __amdgpu_buffer_rsrc_t dst;   // rows [r0, rend)
    int r0, R1;
    uint32_t in;
};
template <int E>
__device__ __forceinline__ void bp_unpack_event(const BPUnpack &U, const StencilArgs &a, int ev) {
    const int lane = threadIdx.x & 63;
    const lds_u32x4 *rd = (const lds_u32x4 *)(uintptr_t)(U.in + E * PairRing<4>::SLOT + 16 * lane);
    const u32x4 va = rd[0], vb = rd[64];
    const int y = U.r0 + 2 * ev;
    const int64_t pb = a.pitch * 4;
    const uint32_t oa = y < U.R1 ? (uint32_t)((y - U.r0) * pb) : kOOB;
    const uint32_t ob = y + 1 < U.R1 ? (uint32_t)((y + 1 - U.r0) * pb) : kOOB;
    uint32_t w[4], x[32];
    w[0] = va.x, w[1] = va.y, w[2] = va.z, w[3] = va.w;
    bp_unpack(w, x);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t t[4] = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
        buf_store<4>(U.dst, U.st[q] + oa, t);
    }
    w[0] = vb.x, w[1] = vb.y, w[2] = vb.z, w[3] = vb.w;
    bp_unpack(w, x);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t t[4] = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
        buf_store<4>(U.dst, U.st[q] + ob, t);
    }
    if constexpr (E & 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
template <int... E>
__device__ __forceinline__ void bp_unpack_trip(const BPUnpack &U, const StencilArgs &a, int ev,
                                               std::integer_sequence<int, E...>) {
    (bp_unpack_event<E>(U, a, ev + E), ...);
}

// KE > 0: the pack and the unpack run inside the first and the last wave, each
// also running KE pair stages (pair_event IN = 2 / OUT = 2), so every wave of
// the workgroup computes: K = 8·S + 2·KE.
template <int S, int KE = 0>
__global__ __launch_bounds__(64 * (S + 2)) __attribute__((amdgpu_waves_per_eu(S == 2 ? 1 : 2)))   // (S = 2: LDS-bound)
void bytepair_chain_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    constexpr int KW = 8, K = KW * S + 2 * KE, LAG = chain_lag<KW>();
    using R = PairRing<4>;
    __shared__ __attribute__((aligned(16))) uint8_t bring[kPairSlots * 2 * kBPRow];   // the pack wave's byte rows
    __shared__ __attribute__((aligned(16))) uint8_t ring[S + 1][R::WAVE];   // pair wave s's input; [S]: unpack's
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    int strip, r0, r1, r2;
    if (!chain_item(a, q, nstrips, xcd_remap(blockIdx.x, nblocks), strip, r0, r1, r2)) return;   // (uniform)
    const int T = (int)((a.active_cols + 127) / 128);
    const int64_t pb = a.pitch * 4;
    const bool fs = q.fold && strip == nstrips - 1;
    int b, lo, hi;
    if (q.fold) strip_geometry_fold(T, strip, b, lo, hi);
    else strip_geometry(T, strip, b, lo, hi);
    const int64_t unit = b + (fs ? (lane & 31) : lane);
    bool stored = unit >= lo && unit < hi;
    uint32_t mask[4], all = 0xffffffffu;   // live cells per word (word j bit i: column 128·unit + 4i + j)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t n = (a.active_cols - (128 * unit + j) + 3) / 4;
        mask[j] = n <= 0 ? 0u : (n >= 32 ? 0xffffffffu : ((1u << n) - 1u));
        all &= mask[j];
    }
    const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
    const int rend = fs ? r2 : r1;
    constexpr int M = 2 * K + 2;
    const bool edge = !(full && r0 - M >= a.row_lo && rend + M <= a.row_hi);
    // the folded strip: both half-waves in one pass (lanes 32-63: rows + h), or,
    // near the dead row boundary, lanes 0-31 walk [r0, r2) alone
    int64_t dB = 0;
    int R1 = r1;
    if (fs && !edge) dB = lane >= 32 ? (int64_t)(r1 - r0) * pb : 0;
    else if (fs) stored = stored && lane < 32, R1 = r2;
    if constexpr (KE > 0) {
        // wave w: KW_w stages (KE for the edge waves), rows extended by the later
        // waves' stages, starting chain_lag(writer) events after its writer
        constexpr int LE = chain_lag<KE>();
        auto ext_of = [&](int v) { return v == 0 ? KW * S + KE : (v <= S ? KW * (S - v) + KE : 0); };
        auto start_of = [&](int v) { return v == 0 ? 0 : (v <= S ? LE + LAG * (v - 1) : LE + LAG * S); };
        auto kw_of = [&](int v) { return (v == 0 || v == S + 1) ? KE : KW; };
        int total = 0;
#pragma unroll
        for (int v = 0; v < S + 2; ++v)
            total = max(total, (start_of(v) + chain_wave_events(R1 - r0 + 2 * ext_of(v), kw_of(v))) / 2);
        const int ext = ext_of(w);
        Strip<4> st;
        st.R0 = r0 - ext;
        st.R1 = R1 + ext;
        st.base_row = st.R0 - kw_of(w);   // the first wave: r0 - K, the window's first row
#pragma unroll
        for (int j = 0; j < 4; ++j) st.mask[j] = mask[j];
        LdsRing L;
        L.hi = false;
        L.dma_off = kOOB;
        const int pre = start_of(w) / 2;
        if (w == 0) {   // KE stages on the packed byte rows
            const int64_t c = 128 * unit;
            st.ld_off = c + 128 <= pb ? (uint32_t)(c + dB) : kOOB;
            const uint8_t *sb = static_cast<const uint8_t *>(a.src) + (int64_t)st.base_row * pb;
            const uint64_t sa = reinterpret_cast<uint64_t>(sb);
            st.src4.x = __builtin_amdgcn_readfirstlane((uint32_t)sa);
            st.src4.y = __builtin_amdgcn_readfirstlane((uint32_t)(sa >> 32) & 0xffffu);
            st.src4.z = (uint32_t)((int64_t)(rend - r0 + 2 * K) * pb);
            st.src4.w = 0x00020000u;
            L.lds = (uint32_t)(uintptr_t)&bring[0];
            L.next = (uint32_t)(uintptr_t)&ring[0][0];
            if (edge) chain_wave<KE, true, 2, 1>(st, a, L, pre, total);
            else chain_wave<KE, false, 2, 1>(st, a, L, pre, total);
        } else if (w <= S) {
            L.lds = (uint32_t)(uintptr_t)&ring[w - 1][0];
            L.next = (uint32_t)(uintptr_t)&ring[w][0];
            if (edge) chain_wave<KW, true, 1, 1>(st, a, L, pre, total);
            else chain_wave<KW, false, 1, 1>(st, a, L, pre, total);
        } else {        // KE stages, then the unpack and the byte stores
            const int64_t c = 128 * unit;
            st.st_off = (stored && c + 128 <= pb) ? (uint32_t)(c + dB) : kOOB;
            st.dst_out = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)r0 * pb, 0,
                                                           (int)((int64_t)(rend - r0) * pb), 0x00020000);
            L.lds = (uint32_t)(uintptr_t)&ring[S][0];
            if (edge) chain_wave<KE, true, 1, 2>(st, a, L, pre, total);
            else chain_wave<KE, false, 1, 2>(st, a, L, pre, total);
        }
        return;
    }
    // barriers: every wave runs `total` (the largest of the waves' start + events / 2)
    auto ne_pair = [&](int s) { return chain_wave_events(R1 - r0 + 2 * KW * (S - 1 - s), KW); };
    const int NU = ((R1 - r0 + 1) / 2 + kPairSlots - 1) / kPairSlots * kPairSlots;
    int total = (kBPLagIn + LAG * S + NU) / 2;
#pragma unroll
    for (int s = 0; s < S; ++s) total = max(total, (kBPLagIn + LAG * s + ne_pair(s)) / 2);
    if (w == 0) {   // pack
        BPPack P;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) {
            const int64_t c = 128 * unit + 16 * qq;
            P.ld[qq] = c + 16 <= pb ? (uint32_t)(c + dB) : kOOB;
        }
        P.base = r0 - K;
        P.lim = rend + K;
        const uint8_t *sb = static_cast<const uint8_t *>(a.src) + (int64_t)P.base * pb;
        const uint64_t sa = reinterpret_cast<uint64_t>(sb);
        P.src4.x = __builtin_amdgcn_readfirstlane((uint32_t)sa);
        P.src4.y = __builtin_amdgcn_readfirstlane((uint32_t)(sa >> 32) & 0xffffu);
        P.src4.z = (uint32_t)((int64_t)(rend - r0 + 2 * K) * pb);
        P.src4.w = 0x00020000u;
        P.bring = (uint32_t)(uintptr_t)&bring[0];
        P.out = (uint32_t)(uintptr_t)&ring[0][0];
        const int NE = ne_pair(0);
#pragma unroll
        for (int e = 0; e < kPairSlots - 1; ++e)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int rr = P.base + 2 * e + r;
                const uint32_t ro = (rr >= a.row_lo && rr < a.row_hi) ? (uint32_t)((rr - P.base) * pb) : kOOB;
#pragma unroll
                for (int qq = 0; qq < 8; ++qq)
                    dma_pair(P.src4, P.ld[qq] + ro, P.bring + e * 2 * kBPRow + r * kBPRow + 1024 * qq);
            }
        for (int ev = 0; ev < NE; ev += kPairSlots)
            bp_pack_trip(P, a, ev, std::make_integer_sequence<int, kPairSlots>{});
        for (int d = NE / 2; d < total; ++d) asm volatile("s_barrier" ::: "memory");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA into LDS outlives the wave
    } else if (w <= S) {   // pair wave s = w - 1
        const int s = w - 1;
        const int ext = KW * (S - 1 - s);
        Strip<4> st;
        st.R0 = r0 - ext;
        st.R1 = R1 + ext;
        st.base_row = st.R0 - KW;
#pragma unroll
        for (int j = 0; j < 4; ++j) st.mask[j] = mask[j];
        LdsRing L;
        L.lds = (uint32_t)(uintptr_t)&ring[s][0];
        L.next = (uint32_t)(uintptr_t)&ring[s + 1][0];
        L.hi = false;
        L.dma_off = kOOB;
        u32x2 o;
        o.x = o.y = kOOB;   // (the lane offsets the events read back: unused without DMA and stores)
        *(lds_u32x2 *)(uintptr_t)(L.lds + R::OFFS + lane * 8) = o;
        const int pre = (kBPLagIn + LAG * s) / 2;
        if (edge) chain_wave<KW, true, 1, 1>(st, a, L, pre, total);
        else chain_wave<KW, false, 1, 1>(st, a, L, pre, total);
    } else {   // unpack
        BPUnpack U;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) {
            const int64_t c = 128 * unit + 16 * qq;
            U.st[qq] = (stored && c + 16 <= pb && c < a.active_cols) ? (uint32_t)(c + dB) : kOOB;
        }
        U.dst = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)r0 * pb, 0,
                                                  (int)((int64_t)(rend - r0) * pb), 0x00020000);
        U.r0 = r0;
        U.R1 = R1;
        U.in = (uint32_t)(uintptr_t)&ring[S][0];
        const int pre = (kBPLagIn + LAG * S) / 2;
        for (int d = 0; d < pre; ++d) asm volatile("s_barrier" ::: "memory");
        for (int ev = 0; ev < NU; ev += kPairSlots)
            bp_unpack_trip(U, a, ev, std::make_integer_sequence<int, kPairSlots>{});
        for (int d = pre + NU / 2; d < total; ++d) asm volatile("s_barrier" ::: "memory");
    }
}

// The bit kernel: one wave per (strip, chunk) item, 2 words (one 64-column
// group) per lane, so the K=7 pipeline fits 128 VGPRs = 4 waves per SIMD.
// NCH stage chains, RING load-ring rows (see BitState).  V = G = 4: the same on
// the 4-word-group layout of a k = 8 context (its short blocks and bands).
template <int K, int NCH, int RING, int AUX, int V = 2, int G = kGroupWords, bool PLAIN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(G == 4 ? 2 : 4)))
void bit_pipe_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    auto body = [&](int strip, int r0, int r1) {
        Strip<V> st;
        st.setup(a, K, strip, r0, r1, 0u);
        constexpr int CL = (K + NCH - 1) / NCH;
        // chunks whose light cone stays inside the live rows, in strips whose cells
        // are all inside the grid, skip the per-row checks and the column masks
        constexpr int M = 2 * K + (K - 1) / CL;
        uint32_t all = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < V; ++j) all &= st.mask[j];
        const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
        if (full && st.R0 - M >= a.row_lo && st.R1 + M <= a.row_hi) bit_run<V, K, CL, RING, AUX, false, G>(st, a);
        else bit_run<V, K, CL, RING, AUX, true, G>(st, a);
    };
    if constexpr (PLAIN) for_each_item_plain(a, q, nstrips, nblocks, body);
    else for_each_item(a, q, nstrips, nblocks, body);
}

// --------------------------------------------------------------- byte layout
// V dwords = 4V cells per lane (V = 4: one 1-KiB row segment per wave).
// Vertical sums first (v_add3 of 3 rows), then horizontal byte shifts of the
// vertical sums.  RING = load-ring rows (prefetch distance RING/2).
// (Aligned strips for k = 1 — every lane stores whole 128-B lines, the two cells
// beyond the segment from one extra dword per row — helped 16-B lanes but lost
// 7 % on the 8-B lanes kept: profiles/r03b_byte1_ab.jsonl; code at commit
// 1e18562, GOL_BYTE1_ALIGN.)

template <int K, int V, int RING>
struct ByteState {
    uint32_t c[K][3][V];
    uint32_t ld[RING][V];
};

// s8 = 9-sum − self; next = ((s8 | alive) == 3), SWAR over 4 bytes (values < 16).
__device__ __forceinline__ uint32_t life_bytes(uint32_t t9, uint32_t alive, uint32_t mask) {
    const uint32_t s8 = t9 - alive;
    const uint32_t y = (s8 | alive) ^ 0x03030303u;
    const uint32_t z = y + 0x7f7f7f7fu;
    return (~z >> 7) & mask;   // mask ⊆ 0x01010101
}

template <int K, int V, int RING, bool EDGE, int P>
__device__ __forceinline__ void byte_phase(ByteState<K, V, RING> &S, const Strip<V> &st, const StencilArgs &a, int it,
                                           int N) {
    constexpr int PD = RING / 2;
    const int rho = st.R0 - K + it;
    uint32_t nv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) nv[j] = S.ld[P % RING][j];
    const uint32_t roff = (it + PD < N) ? st.row_off(a, rho + PD) : kOOB;
    buf_load<V>(S.ld[(P + PD) % RING], st.src, st.ld_off + roff);
    constexpr int A = (P + 1) % 3, B = (P + 2) % 3, C = P % 3;
#pragma unroll
    for (int g = 0; g < K; ++g) {
        uint32_t vs[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            S.c[g][C][j] = nv[j];
            vs[j] = S.c[g][A][j] + S.c[g][B][j] + nv[j];   // v_add3_u32, bytes <= 3
        }
        const uint32_t lft = __builtin_amdgcn_update_dpp(0u, vs[V - 1], 0x138, 0xf, 0xf, true);
        const uint32_t rgt = __builtin_amdgcn_update_dpp(0u, vs[0], 0x130, 0xf, 0xf, true);
        const int x = rho - g - 1;
        const bool valid = !EDGE || (x >= a.row_lo && x < a.row_hi);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t pv = j == 0 ? lft : vs[j - 1];
            const uint32_t nx = j == V - 1 ? rgt : vs[j + 1];
            const uint32_t t9 = funnel(vs[j], pv, 24) + vs[j] + funnel(nx, vs[j], 8);
            const uint32_t o = life_bytes(t9, S.c[g][B][j], st.mask[j]);
            nv[j] = valid ? o : 0u;
        }
    }
    const uint32_t soff = (it >= 2 * K && it < N) ? (uint32_t)((rho - K - st.base_row) * (int)(a.pitch * 4)) : kOOB;
    buf_store<V>(st.dst, st.st_off + soff, nv);
}

template <int K, int V, int RING, bool EDGE, int... P>
__device__ __forceinline__ void byte_phases(ByteState<K, V, RING> &S, const Strip<V> &st, const StencilArgs &a, int it,
                                            int N, std::integer_sequence<int, P...>) {
    (byte_phase<K, V, RING, EDGE, P>(S, st, a, it + P, N), ...);
}

template <int K, int V, int RING, bool EDGE>
__device__ __forceinline__ void byte_run(const Strip<V> &st, const StencilArgs &a) {
    ByteState<K, V, RING> S;
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < V; ++j) S.c[g][s][j] = 0u;
    const int N = (st.R1 - st.R0) + 2 * K;
#pragma unroll
    for (int s = 0; s < RING / 2; ++s) {
        const uint32_t roff = s < N ? st.row_off(a, st.R0 - K + s) : kOOB;
        buf_load<V>(S.ld[s], st.src, st.ld_off + roff);
    }
    constexpr int U = RING % 3 == 0 ? RING : 3 * RING;
    for (int it = 0; it < N; it += U)   // iterations past N are harmless: no loads, no stores
        byte_phases<K, V, RING, EDGE>(S, st, a, it, N, std::make_integer_sequence<int, U>{});
}

template <int K, int V = 4, int RING = 6, bool PLAIN = false>
__global__ __launch_bounds__(256) void byte_pipe_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    auto body = [&](int strip, int r0, int r1) {
        Strip<V> st;
        st.setup(a, K, strip, r0, r1, 0x01010101u);
        if (st.R0 - 2 * K >= a.row_lo && st.R1 + 2 * K <= a.row_hi) byte_run<K, V, RING, false>(st, a);
        else byte_run<K, V, RING, true>(st, a);
    };
    if constexpr (PLAIN) for_each_item_plain(a, q, nstrips, nblocks, body);
    else for_each_item(a, q, nstrips, nblocks, body);
}

// ----------------------------------------------- byte layout, bit-sliced core
// The board stays byte-per-cell in HBM (the reference's bool board: 1 B/cell
// read + 1 B/cell written per launch), but a wave packs each row it loads into
// bit planes, runs the K-stage bit pipeline of the bit layout on them and
// unpacks the output row to bytes before storing it.  The bit core costs
// 15-20 issue slots per 32 cell-updates instead of ~3.5 per cell for byte
// SWAR, so the byte board can afford K = 16-24 generations per HBM pass.
//
// Geometry <V, K>: a lane holds 16·NB columns (NB = 2V dwordx4 loads per row).
//   V = 2 (K <= 16): 4 blocks per wave; lane i of block q holds the 16 columns
//     c0 + S·q + 16i + t, so every load instruction is one coalesced 1-KiB row
//     segment.  HL = ceil(K/16) lanes at each block edge are halo (their outer
//     neighbours are the DPP zero fill; K generations of garbage stay inside
//     their 16·HL columns); blocks overlap by 2·HL lanes (stride
//     S = 16·(64 - 2·HL)), so the strip stores 4·S contiguous columns.  In
//     registers: two words, one 8-bit field per block, bit 8q + j of word w =
//     column t = 2j + w; the left neighbour of word 0 is word 1 shifted up a
//     bit, the right neighbour of word 1 is word 0 shifted down a bit, and the
//     field-end bits come from the adjacent lane (DPP) via a v_bitop3 select.
//   V = 1 (K = 20..32): lane i holds the 32 contiguous columns c0 + 32i + t in
//     one word (bit t), loaded as two 16-B halves (32-B lane stride); lanes 0
//     and 63 are halo (32 columns >= K), the strip stores 62·32 = 1984 columns.
//     Neighbours: funnel shifts with the adjacent lane's word (DPP).
//     Half the per-stage state of V = 2, so K = 24 fits 2 waves/SIMD.
template <int V, int K>
struct BBGeom {
    static constexpr int NB = 2 * V;                          // 16-B loads per lane and row
    static constexpr int HL = V == 2 ? (K + 15) / 16 : (K + 31) / 32;   // halo lanes per edge
    static constexpr int LS = V == 2 ? 16 : 32;               // lane stride (columns)
    static constexpr int S = V == 2 ? 16 * (64 - 2 * HL) : 16;   // load (block / half) stride (columns)
    static constexpr int W = V == 2 ? NB * S : 32 * (64 - 2 * HL);   // columns stored per strip
    static constexpr int NX = 4 * NB;                         // raw dwords per lane and row
    static_assert(K <= 16 * HL * (V == 2 ? 1 : 2), "halo narrower than the light cone");
};
static_assert(BBGeom<2, 16>::W == 3968 && BBGeom<1, 24>::W == 1984, "bytebit geometry");

template <int V, int K>
struct ByteBitStrip {
    using G = BBGeom<V, K>;
    uint32_t ld_off[G::NB], st_off[G::NB];   // row-relative byte offsets per block (kOOB: outside)
    uint32_t mask[V];                        // live cells per word
    int R0, R1, base_row;
    __amdgpu_buffer_rsrc_t src, dst;

    __device__ __forceinline__ void setup(const StencilArgs &a, int strip, int r0, int r1) {
        const int lane = threadIdx.x & 63;
        const int64_t pitch_b = a.pitch * 4;
        const int64_t c0 = (int64_t)strip * G::W - G::LS * G::HL;
#pragma unroll
        for (int w = 0; w < V; ++w) mask[w] = 0u;
#pragma unroll
        for (int q = 0; q < G::NB; ++q) {
            const int64_t col = c0 + G::S * q + G::LS * lane;
            const bool in = col >= 0 && col + 16 <= pitch_b;
            ld_off[q] = in ? (uint32_t)col : kOOB;
            st_off[q] = (in && lane >= G::HL && lane < 64 - G::HL && col < a.active_cols) ? (uint32_t)col : kOOB;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int64_t cc = col + t;
                if (cc >= 0 && cc < a.active_cols) {
                    if constexpr (V == 2) mask[t & 1] |= 1u << (8 * q + (t >> 1));
                    else mask[0] |= 1u << (16 * q + t);   // q = half of the lane's 32 columns
                }
            }
        }
        R0 = r0;
        R1 = r1;
        base_row = R0 - K;
        const int win_rows = R1 - R0 + 2 * K;
        const int nrec = (int)(win_rows * pitch_b);
        src = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t *>(static_cast<const uint8_t *>(a.src)) + (int64_t)base_row * pitch_b, 0, nrec,
            0x00020000);
        dst = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)base_row * pitch_b, 0,
                                                nrec, 0x00020000);
    }
    __device__ __forceinline__ uint32_t row_off(const StencilArgs &a, int rr) const {
        return (rr >= a.row_lo && rr < a.row_hi) ? (uint32_t)((rr - base_row) * (int)(a.pitch * 4)) : kOOB;
    }
};

// Window slots per stage: three rotating slots (phase P writes slot P % 3), or
// two (ROT2: the new row's sums go to temporaries and overwrite the older slot
// after the rule).  The compiler keeps all three slots of every stage live
// across the unrolled loop — 8 VGPRs per stage — but only two of ROT2's
// (≈6.2 per stage, no extra instructions): K = 32 fits 237 VGPRs = 2 waves/SIMD
// (256 + 18 AGPRs = 1 wave/SIMD with three slots).  ROT2 needs a 6-phase trip
// (load ring period 3 × slot period 2), twice the code: at K <= 28, which fit
// either way, the 3-phase loop is kept (ROT2 cost 11 % at 16384², where short
// chunks make the warm-up-level loops hot too; tie at 32768²,
// profiles/r04h_byte_rot2_ab.jsonl, profiles/r04i_byte16k_ab.jsonl).
template <int K>
constexpr bool bb_rot2() { return K >= 32; }
template <int K>
constexpr int bb_trip_len() { return bb_rot2<K>() ? 6 : 3; }

template <int V, int K>
struct ByteBitState {
    uint32_t h0[K][3][V], h1[K][3][V], c[K][3][V];
    uint32_t ld[3][BBGeom<V, K>::NX];   // 3-row load ring of raw 0/1 bytes
};
// (Two interleaved stage chains for the two-slot pipeline — stages [K/2, K) on
// the rows stages [0, K/2) produced one iteration earlier, ILP for one more
// register and warm-up row — ran 6 % slower at K = 32, tie at 28:
// profiles/r04n_bbfold_bbch2_ab.jsonl; code at commit 1e18562, GOL_BB_CHAINS.)

// V = 2: 16 dwords of 0/1 bytes (block q, dword d: columns 16i + 4d + byte) -> 2 words.
__device__ __forceinline__ void bb_pack(const uint32_t (&x)[16], uint32_t (&w)[2]) {
    uint32_t u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        // byte b of z: cells 4d+b at bits 2d; word w's field = byte w | byte w+2 << 1
        const uint32_t z = x[4 * q] | (x[4 * q + 1] << 2) | (x[4 * q + 2] << 4) | (x[4 * q + 3] << 6);
        u[q] = z | (z >> 15);
    }
    const uint32_t A = __builtin_amdgcn_perm(u[1], u[0], 0x05010400u);   // u0.b0 u1.b0 u0.b1 u1.b1
    const uint32_t B = __builtin_amdgcn_perm(u[3], u[2], 0x05010400u);
    w[0] = __builtin_amdgcn_perm(B, A, 0x05040100u);
    w[1] = __builtin_amdgcn_perm(B, A, 0x07060302u);
}

// V = 1: 8 dwords (the lane's two 16-column halves q) -> 1 word, bit 16q + t.
__device__ __forceinline__ void bb_pack(const uint32_t (&x)[8], uint32_t (&w)[1]) {
    uint32_t f[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        // y: byte b holds cells 4·0+b (bit 0) and 4·1+b (bit 4); z: cells 8+b, 12+b.
        // Gathering byte b down by 7b bits puts them at bits b and 4+b.
        const uint32_t y = x[4 * q] | (x[4 * q + 1] << 4);
        const uint32_t z = x[4 * q + 2] | (x[4 * q + 3] << 4);
        const uint32_t gy = y | (y >> 7) | (y >> 14) | (y >> 21);
        const uint32_t gz = z | (z >> 7) | (z >> 14) | (z >> 21);
        f[q] = (gy & 0xffu) | ((gz & 0xffu) << 8);
    }
    w[0] = f[0] | (f[1] << 16);
}

// V = 2: 2 words -> 16 dwords of 0/1 bytes (inverse of bb_pack).
__device__ __forceinline__ void bb_unpack(const uint32_t (&w)[2], uint32_t (&x)[16], uint32_t hi16) {
    const uint32_t P01 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u);   // (w0.b0 w1.b0) (w0.b1 w1.b1)
    const uint32_t P23 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u);   // (w0.b2 w1.b2) (w0.b3 w1.b3)
    uint32_t z[4];
    // z: bytes 0/1 = the fields of words 0/1 (even bits: cells 4d+0 / 4d+1),
    // bytes 2/3 = the same fields >> 1 (cells 4d+2 / 4d+3); select by hi16
    z[0] = __builtin_amdgcn_bitop3_b32(P01, P01 << 15, hi16, 0xD8);
    z[1] = __builtin_amdgcn_bitop3_b32(P01 >> 16, P01 >> 1, hi16, 0xD8);
    z[2] = __builtin_amdgcn_bitop3_b32(P23, P23 << 15, hi16, 0xD8);
    z[3] = __builtin_amdgcn_bitop3_b32(P23 >> 16, P23 >> 1, hi16, 0xD8);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 4; ++d) x[4 * q + d] = (z[q] >> (2 * d)) & 0x01010101u;
}

// V = 1: 1 word -> 8 dwords.  Nibble n = cells 4d..4d+3 of a block; spreading
// its bit b to bit 8b is n·(1 + 2^7 + 2^14 + 2^21) (no carries: the partial
// products land on distinct bits) masked to 0x01010101 — a 24-bit multiply.
__device__ __forceinline__ void bb_unpack(const uint32_t (&w)[1], uint32_t (&x)[8], uint32_t) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t n = (w[0] >> (16 * q + 4 * d)) & 0xfu;
            x[4 * q + d] = __umul24(n, 0x204081u) & 0x01010101u;
        }
}

// V = 1 unpack through an LDS table: entry e = the 8 cells of bit byte e as 8
// bytes (two dwords), built once per block; per row 4 ds_read_b64 and 2
// full-rate VALU each instead of 3 VALU per 4 cells (+0.5-1 % at k = 28).
__shared__ u32x2 bb_lut[256];

// Horizontal 3-sums (h0 = L^C^R, h1 = maj) of one row of generation g.
__device__ __forceinline__ void bb_hsum(const uint32_t (&nv)[2], uint32_t (&n0)[2], uint32_t (&n1)[2], uint32_t lo,
                                        uint32_t hi) {
    const uint32_t xl = __builtin_amdgcn_update_dpp(0u, nv[1], 0x138, 0xf, 0xf, true);   // wave_shr:1
    const uint32_t xr = __builtin_amdgcn_update_dpp(0u, nv[0], 0x130, 0xf, 0xf, true);   // wave_shl:1
    const uint32_t L0 = __builtin_amdgcn_bitop3_b32(nv[1] << 1, xl >> 7, lo, 0xD8);   // lo ? xl>>7 : w1<<1
    const uint32_t R1 = __builtin_amdgcn_bitop3_b32(nv[0] >> 1, xr << 7, hi, 0xD8);   // hi ? xr<<7 : w0>>1
    n0[0] = xor3(L0, nv[0], nv[1]);
    n1[0] = maj(L0, nv[0], nv[1]);
    n0[1] = xor3(nv[0], nv[1], R1);
    n1[1] = maj(nv[0], nv[1], R1);
}
__device__ __forceinline__ void bb_hsum(const uint32_t (&nv)[1], uint32_t (&n0)[1], uint32_t (&n1)[1], uint32_t,
                                        uint32_t) {
    const uint32_t xl = __builtin_amdgcn_update_dpp(0u, nv[0], 0x138, 0xf, 0xf, true);   // wave_shr:1
    const uint32_t xr = __builtin_amdgcn_update_dpp(0u, nv[0], 0x130, 0xf, 0xf, true);   // wave_shl:1
    const uint32_t L = funnel(nv[0], xl, 31);   // column t-1: (w << 1) | bit 31 of the left lane
    const uint32_t R = funnel(xr, nv[0], 1);    // column t+1: (w >> 1) | bit 0 of the right lane << 31
    n0[0] = xor3(L, nv[0], R);
    n1[0] = maj(L, nv[0], R);
}

// KA < K: one of the chunk's first iterations, in which only stages [0, KA)
// produce rows that matter (stage g's first needed output is at iteration
// 2g+2, its window rows from 2g on): the later stages and the store are left out.
template <int V, int K, bool EDGE, int P, int KA = K>
__device__ __forceinline__ void bb_phase(ByteBitState<V, K> &S, const ByteBitStrip<V, K> &st, const StencilArgs &a,
                                         int it, int N, uint32_t lo, uint32_t hi, uint32_t hi16) {
    using G = BBGeom<V, K>;
    const int rho = st.R0 - K + it;   // generation-0 row arriving this iteration (loaded 2 iterations ago)
    uint32_t nv[V];
    bb_pack(S.ld[P % 3], nv);
    {   // prefetch row rho+2 (unconditional: OOB reads 0)
        const uint32_t roff = (it + 2 < N) ? st.row_off(a, rho + 2) : kOOB;
#pragma unroll
        for (int q = 0; q < G::NB; ++q) {
            uint32_t t[4];
            buf_load<4>(t, st.src, st.ld_off[q] + roff);
#pragma unroll
            for (int d = 0; d < 4; ++d) S.ld[(P + 2) % 3][4 * q + d] = t[d];
        }
    }
    static_assert(P < bb_trip_len<K>(), "phase outside the trip");
    if constexpr (bb_rot2<K>()) {
    // two window slots per stage: A (older) = slot P%2, B = slot (P+1)%2; the
    // new row's sums go to temporaries and overwrite A after the rule
    constexpr int A = P % 2, B = (P + 1) % 2;
    // stage g: v = generation g, row rho-g -> generation g+1, row rho-g-1
    auto stage = [&](uint32_t(&v)[V], int g) {
        uint32_t t0[V], t1[V];
        bb_hsum(v, t0, t1, lo, hi);
        const int x = rho - g - 1;
        const bool valid = !EDGE || (x >= a.row_lo && x < a.row_hi);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t o = life_bits(S.h0[g][A][j], S.h1[g][A][j], S.h0[g][B][j], S.h1[g][B][j],
                                         t0[j], t1[j], S.c[g][B][j], st.mask[j]);
            S.c[g][A][j] = v[j];
            S.h0[g][A][j] = t0[j];
            S.h1[g][A][j] = t1[j];
            v[j] = valid ? o : 0u;
        }
    };
#pragma unroll
    for (int g = 0; g < KA; ++g) stage(nv, g);
    } else {
    constexpr int A = (P + 1) % 3, B = (P + 2) % 3, C = P % 3;
#pragma unroll
    for (int g = 0; g < KA; ++g) {
        // nv = generation g, row rho-g
        bb_hsum(nv, S.h0[g][C], S.h1[g][C], lo, hi);
#pragma unroll
        for (int j = 0; j < V; ++j) S.c[g][C][j] = nv[j];
        const int x = rho - g - 1;   // generation g+1, row rho-g-1
        const bool valid = !EDGE || (x >= a.row_lo && x < a.row_hi);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t o = life_bits(S.h0[g][A][j], S.h1[g][A][j], S.h0[g][B][j], S.h1[g][B][j],
                                         S.h0[g][C][j], S.h1[g][C][j], S.c[g][B][j], st.mask[j]);
            nv[j] = valid ? o : 0u;
        }
    }
    }
    if constexpr (KA < K) return;
    // generation K, row rho-K: stored when it lies in [R0, R1)  (it in [2K, N))
    const uint32_t roff = (it >= 2 * K && it < N) ? (uint32_t)((rho - K - st.base_row) * (int)(a.pitch * 4)) : kOOB;
    uint32_t out[G::NX];
    if constexpr (V == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x2 e = bb_lut[(nv[0] >> (8 * i)) & 0xffu];
            out[2 * i] = e.x;
            out[2 * i + 1] = e.y;
        }
    } else {
        bb_unpack(nv, out, hi16);
    }
#pragma unroll
    for (int q = 0; q < G::NB; ++q) {
        const uint32_t t[4] = {out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
        buf_store<4>(st.dst, st.st_off[q] + roff, t);
    }
}

// One unrolled trip: the load ring has period 3, the window slots period 3
// (or 2 with ROT2: a 6-phase trip), so every slot index is static.
template <int V, int K, bool EDGE, int KA, int... P>
__device__ __forceinline__ void bb_trip(ByteBitState<V, K> &S, const ByteBitStrip<V, K> &st, const StencilArgs &a,
                                        int it, int N, uint32_t lo, uint32_t hi, uint32_t hi16,
                                        std::integer_sequence<int, P...>) {
    (bb_phase<V, K, EDGE, P, KA>(S, st, a, it + P, N, lo, hi, hi16), ...);
}

template <int V, int K, bool EDGE, int KA, int IT>
__device__ __forceinline__ void bb_level(ByteBitState<V, K> &S, const ByteBitStrip<V, K> &st, const StencilArgs &a,
                                         int &it, int N, uint32_t lo, uint32_t hi, uint32_t hi16) {
    constexpr int T = bb_trip_len<K>();
    for (; it < IT; it += T)
        bb_trip<V, K, EDGE, KA>(S, st, a, it, N, lo, hi, hi16, std::make_integer_sequence<int, T>{});
}
template <int V, int K, bool EDGE, int... L>
__device__ __forceinline__ void bb_levels(ByteBitState<V, K> &S, const ByteBitStrip<V, K> &st, const StencilArgs &a,
                                          int &it, int N, uint32_t lo, uint32_t hi, uint32_t hi16,
                                          std::integer_sequence<int, L...>) {
    constexpr int NL = sizeof...(L) + 1;
    // level l+1: stages [0, K(l+1)/NL) up to iteration 2K(l+1)/NL (a whole number of trips, <= 2·KA)
    constexpr int T = bb_trip_len<K>();
    (bb_level<V, K, EDGE, K * (L + 1) / NL, 2 * (K * (L + 1) / NL) / T * T>(S, st, a, it, N, lo, hi, hi16), ...);
}

template <int V, int K, bool EDGE>
__device__ __forceinline__ void bb_run(const ByteBitStrip<V, K> &st, const StencilArgs &a) {
    using G = BBGeom<V, K>;
    ByteBitState<V, K> S;
#pragma unroll
    for (int g = 0; g < K; ++g)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int j = 0; j < V; ++j) S.h0[g][s][j] = S.h1[g][s][j] = S.c[g][s][j] = 0u;
    // full-rate v_bitop3 needs its constants in VGPRs, not SGPRs: the field-start
    // and field-end bit masks, and the unpack's byte-half select
    uint32_t lo = 0x01010101u, hi = 0x80808080u, hi16 = 0xffff0000u;   // (V = 2 only)
    asm volatile("" : "+v"(lo), "+v"(hi), "+v"(hi16));
    const int N = (st.R1 - st.R0) + 2 * K;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t roff = s < N ? st.row_off(a, st.R0 - K + s) : kOOB;
#pragma unroll
        for (int q = 0; q < G::NB; ++q) {
            uint32_t t[4];
            buf_load<4>(t, st.src, st.ld_off[q] + roff);
#pragma unroll
            for (int d = 0; d < 4; ++d) S.ld[s][4 * q + d] = t[d];
        }
    }
    // warm-up levels l = 1..L-1: iterations [2K(l-1)/L, 2Kl/L) (rounded to whole
    // trips) run stages [0, Kl/L) only — stage g is needed from iteration 2g
    // on, so (L-1)/L of the start-up triangle of skippable stage-iterations is
    // left out (L = 4: 3/4 of it, ~6-7 % of a K=28 chunk's stage work; at K = 32
    // 2, 6 and 8 levels ran 0.3-2 % slower, profiles/r04x_bb_levels_ab.jsonl)
    constexpr int kLevels = 4;
    int it = 0;
    if constexpr (V == 1)
        bb_levels<V, K, EDGE>(S, st, a, it, N, lo, hi, hi16, std::make_integer_sequence<int, kLevels - 1>{});
    constexpr int T = bb_trip_len<K>();
    for (; it < N; it += T)   // iterations past N are harmless: no loads, no stores
        bb_trip<V, K, EDGE, K>(S, st, a, it, N, lo, hi, hi16, std::make_integer_sequence<int, T>{});
}

template <int V, int K>
__global__ __launch_bounds__(256) void bytebit_pipe_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    if constexpr (V == 1) {   // the unpack table: every wave of the block, before any item
        const uint32_t e = threadIdx.x;
        u32x2 v;
        v.x = __umul24(e & 0xfu, 0x204081u) & 0x01010101u;
        v.y = __umul24(e >> 4, 0x204081u) & 0x01010101u;
        bb_lut[e] = v;
        __syncthreads();
    }
    for_each_item(a, q, nstrips, nblocks, [&](int strip, int r0, int r1) {
        ByteBitStrip<V, K> st;
        st.setup(a, strip, r0, r1);
        if (st.R0 - 2 * K >= a.row_lo && st.R1 + 2 * K <= a.row_hi) bb_run<V, K, false>(st, a);
        else bb_run<V, K, true>(st, a);
    });
}

// ---------------------------------- byte layout, bit-sliced core, stage chain
// bytebit_coop_kernel<V, KW, S>: K = S·KW generations per launch on the byte
// board.  One workgroup is one (strip, chunk) item: a CHAIN of S waves over the
// same 64 lanes, wave s running stages [s·KW, (s+1)·KW).
//  * lane i holds 32·V contiguous columns: V = 1 one word (bit t = column t,
//    the bytebit kernel's geometry), V = 2 two words interleaved (word j bit i
//    = column 2i + j, the bit board's 2-word groups: a row's two lane moves and
//    two funnel shifts serve both words, hsum<2, 2>); HL = ceil(K / 32V) lanes
//    at each strip edge are halo;
//  * rows enter wave 0 through an LDS-DMA ring (kCoopSlots rows of 64 lanes ×
//    32V bytes: 2V buffer_load_dwordx4 … lds per row, lane l's 16-B chunk q at
//    1024·q + 16·l, so the lane reads its chunks back conflict-free), are read
//    back with 2V ds_read_b128 and packed;
//  * wave s hands its last stage's row to wave s + 1 through LDS (kCoopHand
//    slots per boundary), which takes it kCoopLag iterations later: wave s's
//    stage-0 input at iteration it is row R0 - K + it - (KW + kCoopLag)·s;
//  * the last wave unpacks (an LDS table: 8 columns per lookup) and stores;
//  * a workgroup barrier after every kCoopLag-th row keeps the chain in step (a
//    slot is written and read in consecutive barrier intervals).
// Why: one wave holding all K stages is register-bound (the K = 32 bytebit
// kernel: 236 VGPRs, 2 waves/SIMD, and K = 32 is the deepest that fits); a
// chain of waves fuses K = 48 or 64 generations per HBM pass (2 B per cell
// per launch either way), and V = 2 halves the lane moves per word.
// Warm-up: stage g = KW·s + gl of wave s is needed from iteration 2g + s on
// (its window rows), so wave s runs no stage before iteration 2KW·s + s and
// then runs in levels as bb_run does.
constexpr int kCoopSlots = 4;                  // LDS-DMA row slots (3 rows of prefetch)
constexpr int kCoopTrip = 4;                   // phases per unrolled trip: ring period 4, hand-off period 4, window parity 2
// rows between a wave and the next, and rows per barrier: 1.  (2 — a barrier per
// two rows over 4 hand-off slots — parity-green but 1.5-5 % slower at every
// depth, and 8 spills at KW = 16: profiles/r06o_lag_ab.jsonl.  The bit board's
// chain gains from the same change: its waves are 4-6× longer per event.)
constexpr int kCoopLag = 1;
constexpr int kCoopHand = 2 * kCoopLag;        // hand-off slots per wave boundary
typedef __attribute__((address_space(3))) uint32_t lds_u32;

template <int V, int K>
struct CoopGeom {
    static constexpr int LS = 32 * V;              // columns per lane
    static constexpr int HL = (K + LS - 1) / LS;   // halo lanes per strip edge
    static constexpr int W = LS * (64 - 2 * HL);   // columns stored per strip
    static constexpr int NQ = 2 * V;               // 16-B chunks per lane and row
    static constexpr int ROW = 64 * LS;            // bytes of one strip row
};
static_assert(CoopGeom<1, 32>::W == 1984 && CoopGeom<1, 64>::W == 1920 && CoopGeom<2, 64>::W == 3968,
              "chain geometry");

template <int V, int K>
struct CoopStrip {
    using G = CoopGeom<V, K>;
    uint32_t ld_off[G::NQ], st_off[G::NQ];   // row-relative byte offsets of the lane's 16-B chunks (kOOB: outside)
    uint32_t mask[V];                         // live cells per word
    int R0, R1, base_row;
    __amdgpu_buffer_rsrc_t dst;
    u32x4 src4;                               // the source window's descriptor (an SGPR quad for the LDS-DMA asm)

    __device__ __forceinline__ void setup(const StencilArgs &a, int strip, int r0, int r1) {
        const int lane = threadIdx.x & 63;
        const int64_t pitch_b = a.pitch * 4;
        const int64_t col = (int64_t)strip * G::W - G::LS * G::HL + G::LS * lane;
#pragma unroll
        for (int q = 0; q < G::NQ; ++q) {
            const int64_t cq = col + 16 * q;
            const bool in = cq >= 0 && cq + 16 <= pitch_b;
            ld_off[q] = in ? (uint32_t)cq : kOOB;
            st_off[q] = (in && lane >= G::HL && lane < 64 - G::HL && cq < a.active_cols) ? (uint32_t)cq : kOOB;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            uint32_t m = 0u;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int64_t cc = col + V * i + j;
                if (cc >= 0 && cc < a.active_cols) m |= 1u << i;
            }
            mask[j] = m;
        }
        R0 = r0;
        R1 = r1;
        base_row = R0 - K;
        const int nrec = (int)((R1 - R0 + 2 * K) * pitch_b);
        const uint8_t *sb = static_cast<const uint8_t *>(a.src) + (int64_t)base_row * pitch_b;
        const uint64_t sa = reinterpret_cast<uint64_t>(sb);
        src4.x = __builtin_amdgcn_readfirstlane((uint32_t)sa);
        src4.y = __builtin_amdgcn_readfirstlane((uint32_t)(sa >> 32) & 0xffffu);   // stride 0
        src4.z = (uint32_t)nrec;
        src4.w = 0x00020000u;
        dst = __builtin_amdgcn_make_buffer_rsrc(static_cast<uint8_t *>(a.dst) + (int64_t)base_row * pitch_b, 0, nrec,
                                                0x00020000);
    }
    __device__ __forceinline__ uint32_t row_off(const StencilArgs &a, int rr) const {
        return (rr >= a.row_lo && rr < a.row_hi) ? (uint32_t)((rr - base_row) * (int)(a.pitch * 4)) : kOOB;
    }
};

template <int V, int KW>
struct CoopState {
    uint32_t h0[KW][2][V], h1[KW][2][V], c[KW][2][V];   // two window slots per stage (bb_rot2)
};

struct CoopLds {
    uint32_t ring;       // LDS byte address of ring slot 0 (wave 0)
    uint32_t hin, hout;  // hand-off slots: from wave s-1 / to wave s+1 (2 × 256·V B each)
    uint32_t lut;        // LDS byte address of the unpack table (256 × 8 B)
};

enum { kCoopHead = 0, kCoopMid = 1, kCoopTail = 2, kCoopSolo = 3 };

// Unpack table entry e (the last wave: 8 columns per lookup).  V = 1: bit b of
// e = column b (bytebit_pipe_kernel's table).  V = 2: e = nibble m of word 0
// (columns 8m, 8m+2, 8m+4, 8m+6) | nibble m of word 1 << 4 (8m+1, ..., 8m+7).
template <int V>
__device__ __forceinline__ u32x2 coop_lut_entry(uint32_t e) {
    u32x2 t;
    if constexpr (V == 1) {
        t.x = __umul24(e & 0xfu, 0x204081u) & 0x01010101u;
        t.y = __umul24(e >> 4, 0x204081u) & 0x01010101u;
    } else {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const uint32_t bit = (e >> ((o & 1) ? 4 + o / 2 : o / 2)) & 1u;
            if (o < 4) lo |= bit << (8 * o);
            else hi |= bit << (8 * (o - 4));
        }
        t.x = lo;
        t.y = hi;
    }
    return t;
}

// V = 2 pack: 16 dwords of 0/1 bytes (x[j] = columns 4j..4j+3) -> word 0 (even
// columns), word 1 (odd).  e = OR x[j] << j over 8 dwords puts column 4j + b at
// bit 8b + j; the outer perfect shuffle of e (byte swap + 3 delta swaps)
// interleaves bytes 0/2 (-> even columns) and 1/3 (-> odd) bit by bit.
__device__ __forceinline__ uint32_t shuffle32(uint32_t x) {
    x = __builtin_amdgcn_perm(x, x, 0x03010200u);                          // bytes b0 b2 b1 b3
    uint32_t t = __builtin_amdgcn_bitop3_b32(x, x >> 4, 0x00F000F0u, 0x28);   // (x ^ x>>4) & m
    x = xor3(x, t, t << 4);
    t = __builtin_amdgcn_bitop3_b32(x, x >> 2, 0x0C0C0C0Cu, 0x28);
    x = xor3(x, t, t << 2);
    t = __builtin_amdgcn_bitop3_b32(x, x >> 1, 0x22222222u, 0x28);
    return xor3(x, t, t << 1);
}
__device__ __forceinline__ void coop_pack(const uint32_t (&x)[16], uint32_t (&w)[2]) {
    uint32_t e0 = x[0], e1 = x[8];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        e0 |= x[j] << j;
        e1 |= x[8 + j] << j;
    }
    const uint32_t z0 = shuffle32(e0), z1 = shuffle32(e1);
    w[0] = __builtin_amdgcn_perm(z1, z0, 0x05040100u);   // low halves: even columns 0..31, 32..63
    w[1] = __builtin_amdgcn_perm(z1, z0, 0x07060302u);   // high halves: odd columns
}
__device__ __forceinline__ void coop_pack(const uint32_t (&x)[8], uint32_t (&w)[1]) { bb_pack(x, w); }

// Stages [0, KA) of this wave on input row v (generation KW·s, row rho).
template <int V, int KW, bool EDGE, int P, int KA>
__device__ __forceinline__ void coop_stages(CoopState<V, KW> &X, uint32_t (&v)[V], int rho, const StencilArgs &a,
                                            const uint32_t (&mask)[V]) {
    constexpr int A = P % 2, B = (P + 1) % 2;   // older / newer window slot (bb_rot2)
#pragma unroll
    for (int g = 0; g < KA; ++g) {
        uint32_t t0[V], t1[V];
        if constexpr (V == 1) bb_hsum(v, t0, t1, 0u, 0u);
        else hsum<2, 2>(v, t0, t1);
        const int x = rho - g - 1;
        const bool valid = !EDGE || (x >= a.row_lo && x < a.row_hi);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t o = life_bits(X.h0[g][A][j], X.h1[g][A][j], X.h0[g][B][j], X.h1[g][B][j], t0[j], t1[j],
                                         X.c[g][B][j], mask[j]);
            X.c[g][A][j] = v[j];
            X.h0[g][A][j] = t0[j];
            X.h1[g][A][j] = t1[j];
            v[j] = valid ? o : 0u;
        }
    }
}

// One row of the chain at iteration `it` (phase P of the trip): input, stages
// [0, KA), output, barrier.  Rows past N load and store nothing.
template <int V, int KW, int S, int ROLE, bool EDGE, int P, int KA>
__device__ __forceinline__ void coop_phase(CoopState<V, KW> &X, const CoopStrip<V, KW * S> &st, const StencilArgs &a,
                                           const CoopLds &L, int s, int it, int N) {
    using G = CoopGeom<V, KW * S>;
    constexpr int K = KW * S, PD = kCoopSlots - 1;
    const int lane = threadIdx.x & 63;
    const int rho = st.R0 - K + it - (KW + kCoopLag) * s;
    uint32_t v[V];
    if constexpr (ROLE == kCoopHead || ROLE == kCoopSolo) {
        // this row's DMAs were issued PD rows ago; NQ·(PD-1) issued since
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G::NQ * (PD - 1)) : "memory");
        const lds_u32x4 *rd = (const lds_u32x4 *)(uintptr_t)(L.ring + P * G::ROW + 16 * lane);
        uint32_t x[4 * G::NQ];
#pragma unroll
        for (int q = 0; q < G::NQ; ++q) {
            const u32x4 t = rd[64 * q];
            x[4 * q] = t.x;
            x[4 * q + 1] = t.y;
            x[4 * q + 2] = t.z;
            x[4 * q + 3] = t.w;
        }
        {   // row rho + PD into the slot read in the previous phase
            const uint32_t roff = (it + PD < N) ? st.row_off(a, rho + PD) : kOOB;
            const uint32_t sl = L.ring + ((P + PD) % kCoopSlots) * G::ROW;
#pragma unroll
            for (int q = 0; q < G::NQ; ++q) dma_pair(st.src4, st.ld_off[q] + roff, sl + 1024 * q);
        }
        coop_pack(x, v);
    } else {
        // the row wave s-1 wrote kCoopLag iterations ago
        const lds_u32 *hin = (const lds_u32 *)(uintptr_t)(L.hin + ((P + kCoopHand - kCoopLag) % kCoopHand) * 256 * V);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = hin[64 * j + lane];
    }
    coop_stages<V, KW, EDGE, P, KA>(X, v, rho, a, st.mask);
    if constexpr (ROLE == kCoopTail || ROLE == kCoopSolo) {
        if constexpr (KA == KW) {   // generation K, row rho - KW: stored when in [R0, R1)
            const int r = rho - KW;
            const uint32_t roff = (r >= st.R0 && r < st.R1 && it < N)
                                      ? (uint32_t)((r - st.base_row) * (int)(a.pitch * 4)) : kOOB;
            const lds_u32x2 *lut = (const lds_u32x2 *)(uintptr_t)L.lut;   // (an LDS pointer: the offset is no flat address)
            // chunk q (16 columns) = two lookups of 8 columns.  V = 1: bytes 2q, 2q+1
            // of the word.  V = 2: byte q of u (columns 16q..16q+7) and of u2
            // (16q+8..16q+15), u / u2 = nibbles 2q / 2q+1 of both words (coop_lut_entry)
            uint32_t lo = v[0], hi = v[0] >> 8;
            if constexpr (V == 2) {
                lo = __builtin_amdgcn_bitop3_b32(v[0], v[1] << 4, 0x0F0F0F0Fu, 0xE4);   // m ? v0 : v1<<4
                hi = __builtin_amdgcn_bitop3_b32(v[0] >> 4, v[1], 0x0F0F0F0Fu, 0xE4);
            }
#pragma unroll
            for (int q = 0; q < G::NQ; ++q) {
                constexpr int sh = V == 1 ? 16 : 8;
                const u32x2 e0 = lut[(lo >> (sh * q)) & 0xffu], e1 = lut[(hi >> (sh * q)) & 0xffu];
                const uint32_t t[4] = {e0.x, e0.y, e1.x, e1.y};
                buf_store<4>(st.dst, st.st_off[q] + roff, t);
            }
        }
    } else {
        lds_u32 *hout = (lds_u32 *)(uintptr_t)(L.hout + (P % kCoopHand) * 256 * V);
#pragma unroll
        for (int j = 0; j < V; ++j) hout[64 * j + lane] = v[j];
    }
    if constexpr (S > 1 && P % kCoopLag == kCoopLag - 1)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int V, int KW, int S, int ROLE, bool EDGE, int KA, int... P>
__device__ __forceinline__ void coop_trip(CoopState<V, KW> &X, const CoopStrip<V, KW * S> &st, const StencilArgs &a,
                                          const CoopLds &L, int s, int it, int N, std::integer_sequence<int, P...>) {
    (coop_phase<V, KW, S, ROLE, EDGE, P, KA>(X, st, a, L, s, it + P, N), ...);
}

// iterations [it, end) (whole trips) with stages [0, KA)
template <int V, int KW, int S, int ROLE, bool EDGE, int KA>
__device__ __forceinline__ void coop_level(CoopState<V, KW> &X, const CoopStrip<V, KW * S> &st, const StencilArgs &a,
                                           const CoopLds &L, int s, int &it, int end, int N) {
    for (; it < end; it += kCoopTrip)
        coop_trip<V, KW, S, ROLE, EDGE, KA>(X, st, a, L, s, it, N, std::make_integer_sequence<int, kCoopTrip>{});
}

template <int V, int KW, int S, int ROLE, bool EDGE>
__device__ __forceinline__ void coop_run(const CoopStrip<V, KW * S> &st, const StencilArgs &a, const CoopLds &L,
                                         int s) {
    using G = CoopGeom<V, KW * S>;
    constexpr int K = KW * S;
    CoopState<V, KW> X;
#pragma unroll
    for (int g = 0; g < KW; ++g)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < V; ++j) X.h0[g][p][j] = X.h1[g][p][j] = X.c[g][p][j] = 0u;
    const int N = (st.R1 - st.R0) + 2 * K + kCoopLag * (S - 1);
    const int NT = (N + kCoopTrip - 1) / kCoopTrip * kCoopTrip;   // every wave of the chain: NT / kCoopLag barriers
    if constexpr (ROLE == kCoopHead || ROLE == kCoopSolo) {
#pragma unroll
        for (int r = 0; r < kCoopSlots - 1; ++r) {
            const uint32_t roff = r < N ? st.row_off(a, st.R0 - K + r) : kOOB;
#pragma unroll
            for (int q = 0; q < G::NQ; ++q) dma_pair(st.src4, st.ld_off[q] + roff, L.ring + r * G::ROW + 1024 * q);
        }
    }
    // stage group l (stages [KW·l/4, KW·(l+1)/4)) first needed at iteration
    // 2(KW·s + KW·l/4) + kCoopLag·s (its window rows)
    auto start = [&](int gl) { return min(NT, (2 * (KW * s + gl) + kCoopLag * s) / kCoopTrip * kCoopTrip); };
    int it = 0;
    if constexpr (S > 1) {   // nothing of this wave is needed yet: the barriers only
        for (const int e = start(0); it < e; it += kCoopLag) asm volatile("s_barrier" ::: "memory");
    }
    coop_level<V, KW, S, ROLE, EDGE, KW / 4>(X, st, a, L, s, it, start(KW / 4), N);
    coop_level<V, KW, S, ROLE, EDGE, KW / 2>(X, st, a, L, s, it, start(KW / 2), N);
    coop_level<V, KW, S, ROLE, EDGE, 3 * KW / 4>(X, st, a, L, s, it, start(3 * KW / 4), N);
    coop_level<V, KW, S, ROLE, EDGE, KW>(X, st, a, L, s, it, NT, N);
    if constexpr (ROLE == kCoopHead || ROLE == kCoopSolo)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA into LDS outlives the wave
}

template <int V, int KW, int S, int WPE>
__global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(WPE)))
void bytebit_coop_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    using G = CoopGeom<V, KW * S>;
    __shared__ __attribute__((aligned(16))) uint8_t ring[kCoopSlots * G::ROW];
    __shared__ __attribute__((aligned(16))) uint32_t hand[(S > 1 ? S - 1 : 1) * kCoopHand * 64 * V];
    __shared__ __attribute__((aligned(16))) u32x2 lut[256];
    for (int e = threadIdx.x; e < 256; e += 64 * S) lut[e] = coop_lut_entry<V>((uint32_t)e);
    __syncthreads();
    // one item per workgroup (plain schedule: band-major, strip-minor, XCD-remapped)
    const int w = xcd_remap(blockIdx.x, nblocks);
    if (w >= q.nitems) return;
    const int cr = w / nstrips, strip = w - cr * nstrips;
    const int r0 = a.out_r0 + cr * q.rows_per;
    if (r0 >= a.out_r1) return;
    const int r1 = min(r0 + q.rows_per, a.out_r1);
    const int s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    CoopStrip<V, KW * S> st;
    st.setup(a, strip, r0, r1);
    CoopLds L;
    L.ring = (uint32_t)(uintptr_t)&ring[0];
    L.hin = (uint32_t)(uintptr_t)&hand[(s > 0 ? s - 1 : 0) * kCoopHand * 64 * V];
    L.hout = (uint32_t)(uintptr_t)&hand[(s < S - 1 ? s : 0) * kCoopHand * 64 * V];
    L.lut = (uint32_t)(uintptr_t)&lut[0];
    constexpr int K = KW * S;
    const bool edge = !(st.R0 - 2 * K >= a.row_lo && st.R1 + 2 * K <= a.row_hi);
    if constexpr (S == 1) {
        if (edge) coop_run<V, KW, S, kCoopSolo, true>(st, a, L, s);
        else coop_run<V, KW, S, kCoopSolo, false>(st, a, L, s);
    } else if (s == 0) {
        if (edge) coop_run<V, KW, S, kCoopHead, true>(st, a, L, s);
        else coop_run<V, KW, S, kCoopHead, false>(st, a, L, s);
    } else if (s == S - 1) {
        if (edge) coop_run<V, KW, S, kCoopTail, true>(st, a, L, s);
        else coop_run<V, KW, S, kCoopTail, false>(st, a, L, s);
    } else {
        if constexpr (S > 2) {
            if (edge) coop_run<V, KW, S, kCoopMid, true>(st, a, L, s);
            else coop_run<V, KW, S, kCoopMid, false>(st, a, L, s);
        }
    }
}

// columns stored per strip of the bytebit kernel for `gens` generations (0: not instantiated)
static inline int bytebit_strip_cols(int gens) {
    switch (gens) {
    case 4: return BBGeom<2, 4>::W;
    case 8: return BBGeom<2, 8>::W;
    case 12: return BBGeom<2, 12>::W;
    case 16: return BBGeom<2, 16>::W;
    case 20: return BBGeom<1, 20>::W;
    case 24: return BBGeom<1, 24>::W;
    case 28: return BBGeom<1, 28>::W;
    case 32: return BBGeom<1, 32>::W;
    case 48: return CoopGeom<1, 48>::W;
    case 56: return 62 * 128;   // (bytepair_chain_kernel<6, 4> only)
    case 64: return CoopGeom<1, 64>::W;
    default: return 0;
    }
}

// ------------------------------------------------------------ launch helpers

static inline int strips_of(const StencilArgs &a, int v) {
    if (v <= 0) {   // byte layout, bit-sliced core: v = -(columns per strip)
        const int w = -v;
        return (int)std::max<int64_t>(1, (a.active_cols + w - 1) / w);
    }
    return strip_count((a.nunits + v - 1) / v);
}

// Waves that can be resident at once for this kernel on the current device
// (occupancy query × CUs × 4 waves per 256-thread block), cached.
static int resident_waves(const void *fn) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(fn, dev);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int blocks = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 256, 0) != hipSuccess || blocks < 1) blocks = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    const int w = blocks * cus * 4;
    cache[key] = w;
    return w;
}

// Workgroups of `threads` threads that can be resident at once (occupancy × CUs), cached.
static int resident_blocks(const void *fn, int threads) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(fn, dev);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int blocks = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, 0) != hipSuccess || blocks < 1) blocks = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    cache[key] = blocks * cus;
    return blocks * cus;
}

// Chunk height rounded up so the unrolled main loop ends exactly on the chunk's
// last row: the pair kernel runs events in trips of kPairSlots (2 rows each)
// after its K-event prologue, the one-row kernel (RING 6) in trips of 6 rows
// over rows + 2K + D iterations.  A trip past the end computes and discards.
static int align_rows(int h, int gens, bool bit) {
    if (!bit) return h;
    int g = 1, c = 0;
    if (gens >= 8) {   // the pair kernel and its chains: events of 2 rows in trips of kPairSlots
        g = 2 * kPairSlots;
    } else if (gens >= 3) {
        g = 6;
        c = (6 - (2 * gens + (gens >= 5 ? 1 : 0)) % 6) % 6;
    }
    return h + ((c - h) % g + g) % g;
}

// Work plan of one launch (one wave per item, 4 per block).
//  chunk_rows > 0    : chunks of that many rows.
//  -99 <= chunk < 0  : chunk = rows covered in exactly r = -chunk_rows rounds of resident waves.
//  chunk <= -100     : guided, -(100 + r) = r rounds of halving chunks (see Sched).
// Chunks never exceed 2^28 bytes of buffer window (kOOB margin).
// fold_units > 0: the kernel's strips follow strip_geometry_fold over that many
// lane-units (when the geometry folds; else the kernel's own geometry).
static Sched plan_items(const StencilArgs &a, int gens, int v, bool bit, const void *fn, int &waves,
                        int &nstrips, int fold_units = 0, int chain = 0, int wpi = 1) {
    Sched q{};
    const int rows = a.out_r1 - a.out_r0;
    q.fold = (fold_units > 0 && fold_gap(fold_units) > 0) ? 1 : 0;
    nstrips = q.fold ? strip_count(fold_units) : strips_of(a, v);
    // strips' worth of work per chunk-row (twice, so the folded strip counts one half)
    const int ns2 = q.fold ? 2 * nstrips - 1 : 2 * nstrips;
    // (a folded item's source window spans two chunks)
    const int max_rows = (int)std::max<int64_t>(1, (int64_t)(1 << 28) / (a.pitch * 4) / (q.fold ? 2 : 1) - 2 * gens);
    // chain > 0: one item per workgroup of `chain` waves (bytebit_coop_kernel): the
    // resident items are the resident workgroups
    // (wpi > 1: an item takes wpi waves of 256-thread workgroups, bit_chain_kernel)
    const int resident = chain > 0 ? resident_blocks(fn, 64 * chain) : resident_waves(fn) / wpi;
    if (chain == 0 && a.chunk_rows <= -100 && rows >= 8 * 16) {
        const int rounds = std::min(8, std::max(1, -a.chunk_rows - 100));
        const int rows_x = (rows + 7) / 8;
        const int cpr = std::max(1, 2 * resident / 8 / ns2);
        double sum = 0, f = 1;
        for (int r = 0; r < rounds; ++r, f *= 0.5) sum += f;
        q.guided = 1;
        q.cpr = cpr;
        q.nrounds = rounds;
        const int h0 = (int)std::ceil(rows_x / (cpr * sum));
        int covered = 0;
        f = 1;
        for (int r = 0; r < rounds; ++r, f *= 0.5) {
            q.h[r] = std::min(max_rows, align_rows(std::max(8, (int)std::ceil(h0 * f)), gens, bit));
            covered += cpr * q.h[r];
        }
        while (covered < rows_x) {   // top up the first round until the band is covered
            const int add = std::min(max_rows - q.h[0], (rows_x - covered + cpr - 1) / cpr);
            if (add <= 0) break;
            q.h[0] += add;
            covered += cpr * add;
        }
        if (covered >= rows_x) {
            const int per_x = q.fold ? fold_items(cpr * rounds, nstrips) : cpr * nstrips * rounds;
            const int nb = 8 * ((per_x + 3) / 4);
            q.nitems = nb * 4;   // every item slot runs its (guided) body once
            q.rows_per = q.h[0];
            waves = nb * 4;
            return q;
        }
        q.guided = 0;   // could not cover the band within the window limit: fall back to static
    }
    int chunk = a.chunk_rows;
    if (chunk <= -100) chunk = -4;
    if (chunk <= 0) {
        const int rounds = chunk < 0 ? -chunk : 1;
        const int per_round = std::max(1, 2 * resident / ns2);
        chunk = std::max(1, (rows + per_round * rounds - 1) / (per_round * rounds));
        // the pair kernel's chunks end on whole trips (rounded up: never more rounds;
        // k=5/6 measured no better aligned, profiles/r02o_rounds_align_ab.jsonl)
        if (gens == 8 || (bit && gens > 8)) chunk = align_rows(chunk, gens, bit);
        // thin launches (a slab's k-row boundary bands): a chunk costs ~2k rows of
        // warm-up, so never cut below 2k rows — fewer, fuller waves beside the
        // interior kernel
        chunk = std::max(chunk, std::min(rows, 2 * gens));
    }
    chunk = std::min(chunk, max_rows);
    q.rows_per = chunk;
    const int nbands = (rows + chunk - 1) / chunk;
    q.nitems = q.fold ? fold_items(nbands, nstrips) : nbands * nstrips;
    waves = q.nitems;
    return q;
}

// fn_plain: the kernel's PLAIN instantiation, launched for plans without
// guided rounds and without the folded strip.
static hipError_t launch_pipe(const void *fn, const StencilArgs &a, int gens, int v, bool bit, hipStream_t s,
                              int fold_units = 0, const void *fn_plain = nullptr) {
    int waves = 0, ns = 0;
    Sched q = plan_items(a, gens, v, bit, fn, waves, ns, fold_units);
    if (q.nitems <= 0) return hipSuccess;
    if (fn_plain && !q.guided && !q.fold) fn = fn_plain;
    int nb = (waves + 3) / 4;
    StencilArgs aa = a;
    void *args[] = {&aa, &q, &ns, &nb};
    return hipLaunchKernel(fn, dim3(nb), dim3(256), args, 0, s);
}

// The bit kernel per fused generation count (tools/tune.py, tools/ab_libs.sh on
// MI355X): HBM-bound k <= 2 prefetch 9-12 rows ahead; k = 5..7 run
// two stage chains (ILP); k = 8 runs row-pair stages fed by the LDS row ring
// (10.3 VALU instructions per word-update instead of 12.1: +10 % GCUPS).
// Plain cache policy throughout: non-temporal loads/stores (AUX 2) lose 8 % at
// k=1 and 3 % at k=8 (the halo lanes and warm-up rows are L2 hits).
// k=1 words per lane (2; 4 = two groups per lane measured 10 % slower)
constexpr int kK1V = 2;
// Group width of a bit-layout context fusing K generations per launch: the
// k = 8 row-pair kernel runs on 4-word (128-column) groups — a lane's two lane
// moves (DPP) and two funnel shifts per row then serve 4 words instead of 2
//  — every other depth on 2-word groups (4 waves/SIMD at k <= 7).
// (The 2-word-group k = 8 pair kernel, bit_pair_kernel<8, 1, 2>, ran 1.5-5.5 %
// slower: profiles/r04c_g4_bench_ab.jsonl; build knob GOL_BIT_G4 at commit 1e18562.)
int bit_group_words(int K) { return K >= 8 ? 4 : 2; }

// Bit layout: depths a launch can fuse (1..8 one wave per item; 16, 32 the chain)
bool bit_depth_supported(int gens) { return (gens >= 1 && gens <= 8) || gens == 16 || gens == 32; }

static const void *bit_kernel(int gens, int gw) {
    if (gw == 4) {   // a k = 8 context: the pair kernel, and its short blocks on the same layout
        switch (gens) {
        case 1: return (const void *)&bit_pipe_kernel<1, 1, 18, 0, 4, 4>;
        case 2: return (const void *)&bit_pipe_kernel<2, 1, 12, 0, 4, 4>;
        case 3: return (const void *)&bit_pipe_kernel<3, 1, 6, 0, 4, 4>;
        case 4: return (const void *)&bit_pipe_kernel<4, 1, 6, 0, 4, 4>;
        case 5: return (const void *)&bit_pipe_kernel<5, 1, 6, 0, 4, 4>;
        case 6: return (const void *)&bit_pipe_kernel<6, 1, 6, 0, 4, 4>;
        case 7: return (const void *)&bit_pipe_kernel<7, 1, 6, 0, 4, 4>;
        case 8: return (const void *)&bit_pair_kernel<8, 1, 4, 4>;   // one stage chain (two: -6 %,
                                                                       // profiles/r04g_g4_variants_ab.jsonl)
        default: return nullptr;
        }
    }
    switch (gens) {
    case 1: return (const void *)&bit_pipe_kernel<1, 1, 18, 0, kK1V>;   // 9 rows of prefetch
    case 2: return (const void *)&bit_pipe_kernel<2, 1, 24, 0>;   // 12 (profiles/r02h_lowk_ring_ab.jsonl)
    case 3: return (const void *)&bit_pipe_kernel<3, 1, 6, 0>;
    case 4: return (const void *)&bit_pipe_kernel<4, 1, 6, 0>;
    case 5: return (const void *)&bit_pipe_kernel<5, 2, 6, 0>;
    case 6: return (const void *)&bit_pipe_kernel<6, 2, 6, 0>;
    case 7: return (const void *)&bit_pipe_kernel<7, 2, 6, 0>;
    default: return nullptr;   // (k = 8 contexts use 4-word groups: above)
    }
}

hipError_t launch_bit_pipe(const StencilArgs &a, int gens, hipStream_t s) {
    if (a.out_r1 <= a.out_r0) return hipSuccess;
    if (a.gw != 2 && a.gw != 4) return hipErrorInvalidValue;
    if (gens == 16 || gens == 32) {   // the chain of pair waves (4-word groups): 4 / S items per workgroup
        if (a.gw != 4) return hipErrorInvalidValue;
        const int S = gens / 8;
        const void *fn = gens == 16 ? (const void *)&bit_chain_kernel<2> : (const void *)&bit_chain_kernel<4>;
        StencilArgs aa = a;
        if (aa.chunk_rows <= -100) aa.chunk_rows = -1;   // (no guided plan for chains: one round)
        int waves = 0, ns = 0;
        Sched q = plan_items(aa, gens, 4, true, fn, waves, ns, (int)((a.nunits + 3) / 4), 0, S);
        if (q.nitems <= 0) return hipSuccess;
        int nb = (q.nitems + 4 / S - 1) / (4 / S);
        void *args[] = {&aa, &q, &ns, &nb};
        return hipLaunchKernel(fn, dim3(nb), dim3(256), args, 0, s);
    }
    const void *fn = bit_kernel(gens, a.gw);
    if (!fn) return hipErrorInvalidValue;
    // the k = 8 pair kernel's strips follow strip_geometry_fold (the folded tail strip)
    // k = 1: 16-row items, whose plain decoding is +0.2-0.5 % of HBM (profiles/r06am_k1_plain_ab.jsonl)
    const void *plain = (gens == 1 && a.gw == 2) ? (const void *)&bit_pipe_kernel<1, 1, 18, 0, kK1V, 2, true> : nullptr;
    return launch_pipe(fn, a, gens, a.gw == 4 ? 4 : (gens == 1 ? kK1V : 2), true, s,
                       (a.gw == 4 && gens == 8) ? (int)((a.nunits + 3) / 4) : 0, plain);
}

bool bytebit_supported(int gens) { return bytebit_strip_cols(gens) > 0; }

// The chain kernel per depth (bytebit_coop_kernel<V, KW, S, waves/SIMD>), or null;
// chain = its waves per workgroup, cols = columns stored per strip.  Measured at
// 32768² (tools/tune.py, interleaved, profiles/r06c_chain_tune.jsonl,
// profiles/r06e_chain_ab.jsonl): k = 48 <1, 12, 4, 4> 69.0-69.3 k GCUPS, k = 64
// <1, 16, 4, 3> 67.9-68.8 k, against 61.5-62.3 k for the one-wave k = 32 kernel;
// at k = 32 / 24 the chain ties / loses 2 % (the launch is at its streaming floor),
// so those depths keep the one-wave kernel by default (GOL_OPT_BYTE_CORE = 3
// forces the chain).  Two-word lanes (V = 2: half the lane moves per word, but
// 16 VGPRs per stage) lost or tied at every depth: k = 32 <2, 8, 4, 3> 52.8 k,
// k = 48 <2, 12, 4, 2> 66.0 k and <2, 8, 6, 3> 49.5 k, k = 64 <2, 8, 8, 2> 68.0 k
// (parity-green; not instantiated).
template <int V, int KW, int S, int WPE>
static const void *coop_pick(int &chain, int &cols) {
    chain = S;
    cols = CoopGeom<V, KW * S>::W;
    return (const void *)&bytebit_coop_kernel<V, KW, S, WPE>;
}
static const void *coop_kernel(int gens, int &chain, int &cols) {
    chain = cols = 0;
    switch (gens) {
    case 24: return coop_pick<1, 12, 2, 4>(chain, cols);
    case 32: return coop_pick<1, 16, 2, 3>(chain, cols);
    case 48: return coop_pick<1, 12, 4, 4>(chain, cols);
    case 64: return coop_pick<1, 16, 4, 3>(chain, cols);
    default: return nullptr;
    }
}

bool bytebit_chain_default(int gens) { return gens >= 48; }

// The byte board through the bit board's pair waves (bytepair_chain_kernel<S>):
// S = gens / 8 pair waves between a pack and an unpack wave.
// waves = S + 2 per workgroup.
static const void *bytepair_kernel(int gens, int &waves) {
    switch (gens) {
    case 16: waves = 4; return (const void *)&bytepair_chain_kernel<2>;
    case 24: waves = 4; return (const void *)&bytepair_chain_kernel<2, 4>;
    case 32: waves = 6; return (const void *)&bytepair_chain_kernel<4>;
    case 48: waves = 8; return (const void *)&bytepair_chain_kernel<6>;
    case 56: waves = 8; return (const void *)&bytepair_chain_kernel<6, 4>;
    default: waves = 0; return nullptr;
    }
}

hipError_t launch_bytebit_pipe(const StencilArgs &a, int gens, hipStream_t s, int core) {
    if (a.out_r1 <= a.out_r0) return hipSuccess;
    if (core == kByteCorePair || gens == 56) {   // one (strip, chunk) item per workgroup of S + 2 waves
        int NW = 0;
        const void *fn = bytepair_kernel(gens, NW);
        if (fn) {
            StencilArgs aa = a;
            if (aa.chunk_rows <= -100) aa.chunk_rows = -1;   // (no guided plan for workgroup items: one round)
            const int T = (int)((a.active_cols + 127) / 128);   // 128-column lane units
            int waves = 0, ns = 0;
            // v = 32: strips of 64 lanes × 32 dwords (a.nunits counts the row's dwords)
            Sched q = plan_items(aa, gens, 32, true, fn, waves, ns, T, NW);
            if (q.nitems <= 0) return hipSuccess;
            int nb = q.nitems;
            void *args[] = {&aa, &q, &ns, &nb};
            return hipLaunchKernel(fn, dim3(nb), dim3(64 * NW), args, 0, s);
        }
    }
    int chain = 0, ccols = 0;
    const void *cfn = coop_kernel(gens, chain, ccols);
    const bool use_chain = cfn && (core == kByteCoreChain || (core == kByteCoreDefault && bytebit_chain_default(gens)) ||
                                   gens > 32);
    if (use_chain) {   // one (strip, chunk) item per workgroup of `chain` waves
        StencilArgs aa = a;
        if (aa.chunk_rows <= -100) aa.chunk_rows = -1;   // (no guided plan for workgroup items: one round)
        int waves = 0, ns = 0;
        Sched q = plan_items(aa, gens, -ccols, false, cfn, waves, ns, 0, chain);
        if (q.nitems <= 0) return hipSuccess;
        int nb = q.nitems;
        void *args[] = {&aa, &q, &ns, &nb};
        return hipLaunchKernel(cfn, dim3(nb), dim3(64 * chain), args, 0, s);
    }
    const void *fn = gens == 4    ? (const void *)&bytebit_pipe_kernel<2, 4>
                     : gens == 8  ? (const void *)&bytebit_pipe_kernel<2, 8>
                     : gens == 12 ? (const void *)&bytebit_pipe_kernel<2, 12>
                     : gens == 16 ? (const void *)&bytebit_pipe_kernel<2, 16>
                     : gens == 20 ? (const void *)&bytebit_pipe_kernel<1, 20>
                     : gens == 24 ? (const void *)&bytebit_pipe_kernel<1, 24>
                     : gens == 28 ? (const void *)&bytebit_pipe_kernel<1, 28>
                     : gens == 32 ? (const void *)&bytebit_pipe_kernel<1, 32>
                                  : nullptr;
    if (!fn) return hipErrorInvalidValue;
    return launch_pipe(fn, a, gens, -bytebit_strip_cols(gens), false, s);
}

// byte k = 1 (BASELINE config 3 at one generation per pass; HBM-bound): lane
// width, load-ring depth and aligned strips (DESIGN.md §3 has the A/B)
// (profiles/r03b_byte1_ab.jsonl, 32768², 3 interleaved rounds: 4 dwords/lane with 3 rows of prefetch
// 5.29-5.52 TB/s; 2 dwords/lane with 9 rows 5.58-5.92 TB/s, at 16-row chunks; aligned strips 5.80-5.87)
constexpr int kByte1V = 2, kByte1Ring = 18;

hipError_t launch_byte_pipe(const StencilArgs &a, int gens, hipStream_t s) {
    if (a.out_r1 <= a.out_r0) return hipSuccess;
    if (gens == 1)
        return launch_pipe((const void *)&byte_pipe_kernel<1, kByte1V, kByte1Ring>, a, 1, kByte1V, false, s, 0,
                           (const void *)&byte_pipe_kernel<1, kByte1V, kByte1Ring, true>);
    const void *fn = gens == 1   ? (const void *)&byte_pipe_kernel<1>
                     : gens == 2 ? (const void *)&byte_pipe_kernel<2>
                     : gens == 3 ? (const void *)&byte_pipe_kernel<3>
                     : gens == 4 ? (const void *)&byte_pipe_kernel<4>
                     : gens == 5 ? (const void *)&byte_pipe_kernel<5>
                     : gens == 6 ? (const void *)&byte_pipe_kernel<6>
                     : gens == 7 ? (const void *)&byte_pipe_kernel<7>
                     : gens == 8 ? (const void *)&byte_pipe_kernel<8>
                                 : nullptr;
    if (!fn) return hipErrorInvalidValue;
    return launch_pipe(fn, a, gens, 4, false, s);
}

// ------------------------------------------------------------------ init
// glibc TYPE_3 additive generator, x_t = x_{t-3} + x_{t-31} (mod 2^32),
// rand() = x >> 1.  Lanes of a wave take 64 units with the SAME segment index t,
// so the jump matrix M_t = A^{t·seg} is wave-uniform (scalar loads).

template <bool BITS>
__global__ __launch_bounds__(256) void init_units_kernel(const InitUnit *__restrict__ units, int nunits,
                                                         const uint32_t *__restrict__ mats, int seg,
                                                         void *dst, int64_t pitch_bytes) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    const InitUnit &U = units[u < nunits ? u : 0];
    uint32_t w[31], r[31];
#pragma unroll
    for (int i = 0; i < 31; ++i) w[i] = U.w[i];
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 31; ++i) r[i] = w[i];
    } else {
        const uint32_t *M = mats + (size_t)t * 961;
#pragma unroll
        for (int i = 0; i < 31; ++i) {
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < 31; ++k) acc += M[i * 31 + k] * w[k];
            r[i] = acc;
        }
    }
    const int start = t * seg;
    int n = U.len - start;
    if (n > seg) n = seg;
    if (u >= nunits) n = 0;
    const int64_t rowoff = U.row * pitch_bytes;
    uint32_t acc = 0;
    for (int base = 0; base < seg; base += 31) {
#pragma unroll
        for (int i = 0; i < 31; ++i) {
            if (base > 0) r[i] += r[(i + 28) % 31];
            const int pos = base + i;
            // (x>>1) % 3 == 0  <=>  (x>>1)·inv(3) mod 2^32 <= 0x55555555
            const uint32_t cell = (pos < n) && ((r[i] >> 1) * 0xAAAAAAABu <= 0x55555555u);
            if (BITS) {
                acc |= cell << (pos & 31);
                if ((pos & 31) == 31) {
                    if (pos - 31 < n) {
                        uint32_t *row = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(dst) + rowoff);
                        row[(U.col0 + start + pos - 31) >> 5] = acc;
                    }
                    acc = 0;
                }
            } else if (pos < n) {
                static_cast<uint8_t *>(dst)[rowoff + U.col0 + start + pos] = (uint8_t)cell;
            }
        }
    }
}

hipError_t launch_init_units(const InitUnit *units, int nunits, const uint32_t *mats, int T, int seg,
                             void *dst, int64_t pitch_bytes, int bit_layout, hipStream_t s) {
    if (nunits <= 0) return hipSuccess;
    dim3 grid((nunits + 255) / 256, T);
    if (bit_layout)
        hipLaunchKernelGGL(init_units_kernel<true>, grid, dim3(256), 0, s, units, nunits, mats, seg, dst,
                           pitch_bytes);
    else
        hipLaunchKernelGGL(init_units_kernel<false>, grid, dim3(256), 0, s, units, nunits, mats, seg, dst,
                           pitch_bytes);
    return hipGetLastError();
}

// ------------------------------------------------------- layout conversion
// Bit layout = groups of gw words (bit_word / bit_pos, gol_internal.h); rows
// are padded to whole 128-column blocks (4 words).

// bytes (window nrows×ncols, leading dim ld) -> bit words of storage rows
// row0.., columns col0..; partially covered words are merged; cells at columns
// >= active_cols are stored as 0.  One thread per word.
__global__ void pack_window_kernel(const uint8_t *__restrict__ bytes, int64_t ld, uint32_t *words,
                                   int64_t pitch, int64_t row0, int64_t col0, int64_t nrows,
                                   int64_t ncols, int64_t active_cols, int gw) {
    const int64_t gc = 32 * gw;   // columns per group
    const int64_t g0 = col0 / gc, g1 = (col0 + ncols - 1) / gc;
    const int64_t nw = (g1 - g0 + 1) * gw;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nw * nrows) return;
    const int64_t r = t / nw, wi = g0 * gw + t % nw;
    uint32_t *pw = words + (row0 + r) * pitch + wi;
    uint32_t v = *pw;
    const uint8_t *src = bytes + r * ld;
    const int64_t cbase = (wi / gw) * gc + (wi % gw);
    for (int j = 0; j < 32; ++j) {
        const int64_t c = cbase + gw * j;
        if (c < col0 || c >= col0 + ncols) continue;
        const uint32_t bit = (c < active_cols && src[c - col0]) ? 1u : 0u;
        v = (v & ~(1u << j)) | (bit << j);
    }
    *pw = v;
}

__global__ void unpack_window_kernel(const uint32_t *__restrict__ words, int64_t pitch, uint8_t *bytes,
                                     int64_t ld, int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int gw) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nrows * ncols) return;
    const int64_t r = t / ncols, c = t % ncols;
    const int64_t gc = col0 + c;
    bytes[r * ld + c] = (words[(row0 + r) * pitch + bit_word(gc, gw)] >> bit_pos(gc, gw)) & 1u;
}

// Linear words (bit i of word w = column 32w+i, as the init kernel writes them)
// -> gw-word groups.  One thread per 128-column block.
__device__ __forceinline__ uint32_t gather_stride2(uint32_t x, int w) {   // bits w, w+2, ... -> 16 bits
    x = (x >> w) & 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    return (x | (x >> 8)) & 0x0000ffffu;
}
__device__ __forceinline__ uint32_t gather_stride4(uint32_t x, int w) {   // bits w, w+4, ... -> 8 bits
    x = (x >> w) & 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000f000fu;
    return (x | (x >> 12)) & 0x000000ffu;
}

__global__ void interleave_rows_kernel(const uint32_t *__restrict__ lin, uint32_t *__restrict__ out,
                                       int64_t pitch, int64_t r0, int64_t nrows, int64_t blocks, int gw) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nrows * blocks) return;
    const int64_t r = r0 + t / blocks, b = t % blocks;
    const uint4 W = *reinterpret_cast<const uint4 *>(lin + r * pitch + b * 4);
    uint4 o;
    if (gw == 4) {   // one 128-column group: word j bit i = column 4i + j = linear word i/8, bit 4(i%8) + j
        o.x = gather_stride4(W.x, 0) | gather_stride4(W.y, 0) << 8 | gather_stride4(W.z, 0) << 16 |
              gather_stride4(W.w, 0) << 24;
        o.y = gather_stride4(W.x, 1) | gather_stride4(W.y, 1) << 8 | gather_stride4(W.z, 1) << 16 |
              gather_stride4(W.w, 1) << 24;
        o.z = gather_stride4(W.x, 2) | gather_stride4(W.y, 2) << 8 | gather_stride4(W.z, 2) << 16 |
              gather_stride4(W.w, 2) << 24;
        o.w = gather_stride4(W.x, 3) | gather_stride4(W.y, 3) << 8 | gather_stride4(W.z, 3) << 16 |
              gather_stride4(W.w, 3) << 24;
    } else {         // two 64-column groups: linear words (x, y) and (z, w)
        o.x = gather_stride2(W.x, 0) | (gather_stride2(W.y, 0) << 16);
        o.y = gather_stride2(W.x, 1) | (gather_stride2(W.y, 1) << 16);
        o.z = gather_stride2(W.z, 0) | (gather_stride2(W.w, 0) << 16);
        o.w = gather_stride2(W.z, 1) | (gather_stride2(W.w, 1) << 16);
    }
    *reinterpret_cast<uint4 *>(out + r * pitch + b * 4) = o;
}

hipError_t launch_interleave_rows(const uint32_t *lin, uint32_t *out, int64_t pitch_words, int64_t r0,
                                  int64_t nrows, int64_t blocks, int gw, hipStream_t s) {
    const int64_t n = nrows * blocks;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(interleave_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lin, out,
                       pitch_words, r0, nrows, blocks, gw);
    return hipGetLastError();
}

hipError_t launch_pack_window(const uint8_t *bytes, int64_t ld, uint32_t *words, int64_t pitch_words,
                              int64_t row0, int64_t col0, int64_t nrows, int64_t ncols,
                              int64_t active_cols, int gw, hipStream_t s) {
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    const int64_t nw = ((col0 + ncols - 1) / (32 * gw) - col0 / (32 * gw) + 1) * gw;
    const int64_t n = nw * nrows;
    hipLaunchKernelGGL(pack_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bytes, ld,
                       words, pitch_words, row0, col0, nrows, ncols, active_cols, gw);
    return hipGetLastError();
}

hipError_t launch_unpack_window(const uint32_t *words, int64_t pitch_words, uint8_t *bytes, int64_t ld,
                                int64_t row0, int64_t col0, int64_t nrows, int64_t ncols, int gw, hipStream_t s) {
    const int64_t n = nrows * ncols;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, words,
                       pitch_words, bytes, ld, row0, col0, nrows, ncols, gw);
    return hipGetLastError();
}

__global__ void normalize_bytes_kernel(uint8_t *base, int64_t pitch, int64_t nrows, int64_t ncols) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nrows * ncols) return;
    uint8_t *p = base + (t / ncols) * pitch + t % ncols;
    *p = *p != 0;
}

hipError_t launch_normalize_bytes(uint8_t *base, int64_t pitch_bytes, int64_t nrows, int64_t ncols, hipStream_t s) {
    const int64_t n = nrows * ncols;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(normalize_bytes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, base, pitch_bytes,
                       nrows, ncols);
    return hipGetLastError();
}

// ------------------------------------------------------------------ clock probe
// MI355X_MICROARCH.md "DVFS give-back": the chip lowers its clock under load
// and the k=8 bit kernel's clock differs between boxes, so bench.py reports the
// clock the timed steps ran at.  s_memtime counts shader cycles, s_memrealtime
// a constant 100 MHz; the wave sleeps between polls (s_sleep 127 ≈ 8k cycles)
// and always exits after max_ticks.
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long *out, const int *stop,
                                                         unsigned long long max_ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long r = r0;
    for (;;) {
        __builtin_amdgcn_s_sleep(127);
        r = __builtin_amdgcn_s_memrealtime();
        if (r - r0 >= max_ticks) break;
        if (__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) break;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        out[0] = t0;
        out[1] = r0;
        out[2] = t1;
        out[3] = r1;
    }
}

hipError_t launch_clock_probe(unsigned long long *out, const int *stop, unsigned long long max_ticks, hipStream_t s) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, s, out, stop, max_ticks);
    return hipGetLastError();
}

// ------------------------------------------------------------------ popcount
// Cells are 0/1 bytes or bits, so popc of every dword counts live cells in both layouts.
__global__ void popcount_kernel(const uint32_t *__restrict__ buf, int64_t pitch_words, int64_t r0,
                                int64_t nrows, int64_t row_words, unsigned long long *acc) {
    const int64_t n = nrows * row_words;
    unsigned long long local = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / row_words, c = t % row_words;
        local += __popc(buf[(r0 + r) * pitch_words + c]);
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc, local);
}

hipError_t launch_popcount(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t row_bytes,
                           unsigned long long *acc, int bit_layout, hipStream_t s) {
    (void)bit_layout;
    const int64_t nrows = r1 - r0, row_words = (row_bytes + 3) / 4;
    if (nrows <= 0) return hipSuccess;
    int64_t blocks = (nrows * row_words + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(popcount_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                       static_cast<const uint32_t *>(buf), pitch_bytes / 4, r0, nrows, row_words, acc);
    return hipGetLastError();
}

// One thread per cell of the column range (the torus ghost margins: at most 64 columns).
// GW: 0 = byte layout, else the bit layout's group width.
// (The torus kernels are templates on GW: the compiler then emits them behind every
// stencil kernel, whose place in the code object stays what it was without them — the
// row-pair kernels are sensitive to it)
template <int GW>
__global__ void popcount_cols_kernel(const uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                     int64_t nrows, int64_t c0, int64_t ncols, unsigned long long *acc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long local = 0;
    if (t < nrows * ncols) {
        const uint8_t *row = buf + (r0 + t / ncols) * pitch_bytes;
        const int64_t c = c0 + t % ncols;
        local = GW ? (reinterpret_cast<const uint32_t *>(row)[bit_word(c, GW)] >> bit_pos(c, GW)) & 1u
                   : (row[c] != 0);
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(acc, local);
}

hipError_t launch_popcount_cols(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t c0,
                                int64_t c1, unsigned long long *acc, int bit_gw, hipStream_t s) {
    const int64_t n = (r1 - r0) * (c1 - c0);
    if (r1 <= r0 || c1 <= c0) return hipSuccess;
    const auto fn = bit_gw == 4 ? popcount_cols_kernel<4> : bit_gw ? popcount_cols_kernel<2> : popcount_cols_kernel<0>;
    hipLaunchKernelGGL(fn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const uint8_t *>(buf),
                       pitch_bytes, r0, r1 - r0, c0, c1 - c0, acc);
    return hipGetLastError();
}

// ------------------------------------------------------------------ torus wrap
// GOL_TORUS rows carry hk ghost columns on either side of the real ones; the
// stencil kernels see an ordinary dead-boundary row of cols + 2·hk columns, and
// after every launch (and every other write of cells) this kernel copies the
// last hk real columns into the left ghost and the first hk into the right one.
// Bit layout: one lane per row.  The ghosts are bit fields inside the row's
// first group and its last one or two, at other bit offsets than their sources
// (row_get_cols / row_put_cols, gol_internal.h); the access is a pitch-strided
// column, a few words per lane whatever the width, so waves of 64 rows in blocks
// of one wave keep the grid as wide as the rows allow.  The stores are
// read-modify-writes of words that also hold real cells: no other lane touches
// this row, and the launch is stream-ordered after the kernel that wrote it.
template <int GW>
__global__ __launch_bounds__(64) void wrap_cols_bit_kernel(uint32_t *buf, int64_t pitch, int64_t r0, int64_t nrows,
                                                           int64_t cols, int hk) {
    constexpr int gw = GW;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= nrows) return;
    uint32_t *row = buf + (r0 + t) * pitch;
    const uint32_t last = row_get_cols(row, cols, hk, gw);   // real columns [cols-hk, cols) at storage + hk
    const uint32_t first = row_get_cols(row, hk, hk, gw);
    row_put_cols(row, 0, hk, gw, last);
    row_put_cols(row, hk + cols, hk, gw, first);
}

// Byte layout: one thread per ghost byte (the margins may start off a dword boundary).
template <int GW = 0>
__global__ __launch_bounds__(256) void wrap_cols_byte_kernel(uint8_t *buf, int64_t pitch, int64_t r0, int64_t nrows,
                                                             int64_t cols, int hk) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows * 2 * hk) return;
    uint8_t *row = buf + (r0 + t / (2 * hk)) * pitch;
    const int j = (int)(t % (2 * hk));
    if (j < hk) row[j] = row[cols + j];   // left ghost <- storage [cols, cols+hk)
    else row[cols + j] = row[j];          // right ghost [cols+hk, cols+2hk) <- storage [hk, 2hk)
}

hipError_t launch_wrap_cols(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t cols, int hk,
                            int bit_gw, hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || hk <= 0) return hipSuccess;
    if (cols < hk || (bit_gw && hk > 32)) return hipErrorInvalidValue;   // the sources must be real columns
    if (bit_gw)
        hipLaunchKernelGGL(bit_gw == 4 ? wrap_cols_bit_kernel<4> : wrap_cols_bit_kernel<2>,
                           dim3((unsigned)((nrows + 63) / 64)), dim3(64), 0, s, static_cast<uint32_t *>(buf),
                           pitch_bytes / 4, r0, nrows, cols, hk);
    else
        hipLaunchKernelGGL(wrap_cols_byte_kernel<0>, dim3((unsigned)((nrows * 2 * hk + 255) / 256)), dim3(256), 0, s,
                           static_cast<uint8_t *>(buf), pitch_bytes, r0, nrows, cols, hk);
    return hipGetLastError();
}

// Torus init: the generator's linear words (column c at bit c) -> gw-word groups
// shifted by the left ghost margin.  One thread per output word.
template <int GW>
__global__ void interleave_rows_shift_kernel(const uint32_t *__restrict__ lin, uint32_t *__restrict__ out,
                                             int64_t pitch, int64_t r0, int64_t nrows, int64_t row_words,
                                             int64_t ncols, int shift) {
    constexpr int gw = GW;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nrows * row_words) return;
    const int64_t r = r0 + t / row_words, w = t % row_words;
    const int64_t base = (w / gw) * 32 * gw + w % gw - shift;   // linear column of bit 0; bit b: base + gw·b
    const uint32_t *src = lin + r * pitch;
    uint32_t o = 0;
    for (int b = 0; b < 32; ++b) {
        const int64_t c = base + (int64_t)gw * b;
        if (c >= 0 && c < ncols) o |= ((src[c >> 5] >> (c & 31)) & 1u) << b;
    }
    out[r * pitch + w] = o;
}

hipError_t launch_interleave_rows_shift(const uint32_t *lin, uint32_t *out, int64_t pitch_words, int64_t r0,
                                        int64_t nrows, int64_t row_words, int64_t ncols, int shift, int gw,
                                        hipStream_t s) {
    const int64_t n = nrows * row_words;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gw == 4 ? interleave_rows_shift_kernel<4> : interleave_rows_shift_kernel<2>,
                       dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lin, out, pitch_words, r0, nrows, row_words,
                       ncols, shift);
    return hipGetLastError();
}

// ------------------------------------------------- life-like rules (B/S notation)
// The rule-generic instantiation of the bit pipeline (gol_set_rule; k = 1..7 on
// 2-word groups): the same Strip, Sched, hsum, load ring and EDGE split as
// bit_pipe_kernel, with the stage of gol_rule.h in place of the B3/S23 truth
// tables.  The rule is a kernel argument of its own; a wave expands the two
// masks once into the stage's 17 uniform coefficient words (SGPRs).  Emitted
// behind every other kernel so that none of them moves.
struct RuleStage {
    RuleTable T;
    template <bool EDGE>
    __device__ __forceinline__ uint32_t apply(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0,
                                              uint32_t c1, uint32_t alive, uint32_t mask) const {
        return rule_bits<EDGE>(T, a0, a1, b0, b1, c0, c1, alive, mask);
    }
};

template <int K, int NCH, int RING, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE)))
void bit_rule_kernel(StencilArgs a, Sched q, int nstrips, int nblocks, RuleMasks rule) {
    constexpr int V = 2, G = 2;
    for_each_item(a, q, nstrips, nblocks, [&](int strip, int r0, int r1) {
        Strip<V> st;
        st.setup(a, K, strip, r0, r1, 0u);
        RuleStage stage;
        stage.T = rule_table(rule.birth, rule.survive);
        constexpr int CL = (K + NCH - 1) / NCH;
        constexpr int M = 2 * K + (K - 1) / CL;   // as bit_pipe_kernel: the chunk's light cone
        const uint32_t all = st.mask[0] & st.mask[1];
        const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
        if (full && st.R0 - M >= a.row_lo && st.R1 + M <= a.row_hi) bit_run<V, K, CL, RING, 0, false, G>(st, a, stage);
        else bit_run<V, K, CL, RING, 0, true, G>(st, a, stage);
    });
}

// Rings and chains per depth start from bit_kernel()'s; waves per SIMD: DESIGN.md §3.
static const void *bit_rule_fn(int gens) {
    switch (gens) {
    case 1: return (const void *)&bit_rule_kernel<1, 1, 18, 4>;
    case 2: return (const void *)&bit_rule_kernel<2, 1, 24, 4>;
    case 3: return (const void *)&bit_rule_kernel<3, 1, 6, 4>;
    case 4: return (const void *)&bit_rule_kernel<4, 1, 6, 4>;
    case 5: return (const void *)&bit_rule_kernel<5, 2, 6, 4>;
    case 6: return (const void *)&bit_rule_kernel<6, 2, 6, 4>;
    case 7: return (const void *)&bit_rule_kernel<7, 2, 6, 4>;
    default: return nullptr;
    }
}

bool bit_rule_supported(int gens, int gw) { return gw == 2 && bit_rule_fn(gens) != nullptr; }

hipError_t launch_bit_rule(const StencilArgs &a, int gens, const RuleMasks &rule, hipStream_t s) {
    if (a.out_r1 <= a.out_r0) return hipSuccess;
    if (!rule_valid(rule.birth, rule.survive)) return hipErrorInvalidValue;
    const void *fn = a.gw == 2 ? bit_rule_fn(gens) : nullptr;
    if (!fn) return hipErrorInvalidValue;   // no fall-back: a depth without a rule kernel is an error
    int waves = 0, ns = 0;
    Sched q = plan_items(a, gens, 2, true, fn, waves, ns);
    if (q.nitems <= 0) return hipSuccess;
    int nb = (waves + 3) / 4;
    StencilArgs aa = a;
    RuleMasks rr = rule;
    void *args[] = {&aa, &q, &ns, &nb, &rr};
    return hipLaunchKernel(fn, dim3(nb), dim3(256), args, 0, s);
}

// ------------------------------------------------------------------------ digest
// gol_digest* (gol_digest.h): a streaming, read-only reduction of a window of
// storage rows × storage columns.  A wave takes items of 64 units along the row
// (a lane = one unit: 16 B of a bit row, 32 B of a byte row, so a wave's load
// is one contiguous 1- or 2-KiB run) times a segment of 64·m rows.  Per item a
// lane computes its window masks and its NL + 1 weights B_i(w) once and keeps
// them down the rows; per block of 64 rows lane j computes A_i of row j, handed
// to the wave through v_readlane as the rows are walked, so a row costs the
// de-interleave (10 word-pair exchanges), one funnel shift and 2·(NL + 1)
// 64×32 multiply-adds per lane, plus one 64×64 multiply per lane and hash lane
// for A_i(r).  Lanes past the last unit read the first unit under a zero mask.
// At the end one wave reduction (__shfl_down) and one 64-bit vector atomicAdd
// per hash lane and wave: integer addition commutes, so the result does not
// depend on the arrival order.  Templates on G (0 = byte), emitted behind every
// other kernel so that none of them moves.
__device__ __forceinline__ uint64_t digest_readlane(uint64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
    return ((uint64_t)hi << 32) | lo;
}

template <int G>
__global__ __launch_bounds__(256) void digest_kernel(const uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                                     int64_t nrows, int64_t grow0, int64_t pc0, int64_t lc0,
                                                     int64_t ncols, int seg_rows, int64_t q0, int64_t nunits,
                                                     unsigned long long *slot) {
    typedef DigestUnit<G> U;
    constexpr int NL = U::NL;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    const DigestShift h = digest_shift_of(pc0, lc0);
    uint64_t acc[2] = {0, 0};
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        const bool on = cb * 64 + lane < nunits;
        const int64_t q = on ? q0 + cb * 64 + lane : q0;
        uint32_t mask[NL];
        uint64_t Bu[2][5];
#pragma unroll
        for (int t = 0; t < NL; ++t) mask[t] = on ? digest_mask(NL * q + t, pc0, pc0 + ncols) : 0u;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t <= NL; ++t) Bu[i][t] = digest_B(i, NL * q + h.dq + t);
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        for (int64_t rs = ra; rs < rb; rs += 64) {
            const uint64_t a0 = digest_A(0, grow0 + rs + lane), a1 = digest_A(1, grow0 + rs + lane);
            const int n = rb - rs < 64 ? (int)(rb - rs) : 64;
            const uint8_t *p = buf + (r0 + rs) * pitch_bytes + q * U::BYTES;
            // four rows' loads are issued before the first is used (one load in flight per wave
            // left the kernel latency-bound at 3 TB/s); a row past the block's last is the last
            // row again under a zero A
            for (int j0 = 0; j0 < n; j0 += 4) {
                uint4 x[4][U::WORDS / 4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u < n ? j0 + u : n - 1;
#pragma unroll
                    for (int v = 0; v < U::WORDS / 4; ++v)
                        x[u][v] = reinterpret_cast<const uint4 *>(p + j * pitch_bytes)[v];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    uint32_t w[U::WORDS];
#pragma unroll
                    for (int v = 0; v < U::WORDS / 4; ++v) {
                        w[4 * v] = x[u][v].x;
                        w[4 * v + 1] = x[u][v].y;
                        w[4 * v + 2] = x[u][v].z;
                        w[4 * v + 3] = x[u][v].w;
                    }
                    uint64_t sum[2] = {0, 0};
                    digest_unit<G>(w, mask, h.s, Bu, sum);
                    const bool live = j0 + u < n;   // (wave-uniform)
                    acc[0] += (live ? digest_readlane(a0, j0 + u) : 0ull) * sum[0];
                    acc[1] += (live ? digest_readlane(a1, j0 + u) : 0ull) * sum[1];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        unsigned long long v = acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0 && v) atomicAdd(slot + i, v);
    }
}

hipError_t launch_digest(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                         int64_t lc0, int64_t ncols, unsigned long long *slot, int bit_gw, hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    if (r0 < 0 || pc0 < 0 || lc0 < 0 || grow0 < 0 || (bit_gw != 0 && bit_gw != 2 && bit_gw != 4))
        return hipErrorInvalidValue;
    const int64_t ucols = bit_gw ? DigestUnit<2>::COLS : DigestUnit<0>::COLS;
    const int64_t q0 = pc0 / ucols, nunits = (pc0 + ncols - 1) / ucols - q0 + 1;
    const int64_t ncb = (nunits + 63) / 64;
    // segments of 64·m rows: as many items as the capped grid has waves where the window
    // allows (the grid is capped as launch_popcount's), longer segments beyond that, so
    // a lane's weights serve up to 512 rows
    constexpr int64_t kMaxBlocks = 4096;
    int64_t m = (nrows + 63) / 64 * ncb / (kMaxBlocks * 4);
    m = m < 1 ? 1 : m > 8 ? 8 : m;
    int seg_rows = (int)(64 * m);
    const int64_t items = ncb * ((nrows + seg_rows - 1) / seg_rows);
    int64_t blocks = (items + 3) / 4;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const auto fn = bit_gw == 4 ? digest_kernel<4> : bit_gw == 2 ? digest_kernel<2> : digest_kernel<0>;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint8_t *>(buf), pitch_bytes, r0,
                       nrows, grow0, pc0, lc0, ncols, seg_rows, q0, nunits, slot);
    return hipGetLastError();
}

// ----------------------------------------------------------------------- density
// gol_density* (gol_density.h): per-tile live-cell counts, the digest kernel's
// streaming shape with a popcount where the digest has a weighted sum.  A wave
// takes items of 64 units along the row (a lane = one unit) times a segment of
// rows; per item a lane computes its window masks and the tile columns of its
// NL + 1 canonical words once and keeps them down the rows; four rows' loads are
// in flight.  A lane adds NL + 1 32-bit counts down the rows of ONE tile row; at a
// tile-row boundary and at the end of the segment they go to the slab's part:
// where every lane's words lie in one tile column (wave-uniform test) the lanes
// that share a tile are first added up by a segmented __shfl_down reduction (tile
// columns ascend with the lane, so a tile's lanes are neighbours) and the first
// lane of each tile issues one 32-bit vector atomicAdd; else a lane folds its own
// neighbouring words and adds per tile column.  Integer addition commutes, so the
// result does not depend on the arrival order.  Where the run is unshifted and
// every unit of the wave is whole and inside one tile (wave-uniform), rows are
// counted on the storage words as they are (density_unit_whole: no
// de-interleave).  Lanes past the last unit read the first unit and count
// nothing.  Templates on G (0 = byte), emitted behind every other kernel so that
// none of them moves.
template <int G>
__global__ __launch_bounds__(256) void density_kernel(const uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                                      int64_t nrows, int64_t trow_off, int64_t pc0, int64_t lc0,
                                                      int64_t ncols, int64_t col0, int64_t tile_rows,
                                                      int64_t tile_cols, int seg_rows, int64_t q0, int64_t nunits,
                                                      uint32_t *__restrict__ part, int64_t ti_base, int64_t ntr,
                                                      int64_t tcols) {
    typedef DigestUnit<G> U;
    constexpr int NL = U::NL;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    const DigestShift h = digest_shift_of(pc0, lc0);
    const int last = h.s ? NL : NL - 1;   // the unit's last canonical word that can hold a cell
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        const bool on = cb * 64 + lane < nunits;
        const int64_t q = on ? q0 + cb * 64 + lane : q0;
        uint32_t mask[NL], acc[NL + 1];
        int64_t tc[NL + 1];
#pragma unroll
        for (int t = 0; t < NL; ++t) mask[t] = on ? digest_mask(NL * q + t, pc0, pc0 + ncols) : 0u;
#pragma unroll
        for (int t = 0; t <= NL; ++t) {
            tc[t] = on ? density_tile_of(NL * q + h.dq + t, col0, tile_cols) : -1;   // (idle lanes: a tile of their own)
            acc[t] = 0u;
        }
        const bool whole = __all(!on || density_is_whole<G>(mask, h.s, tc));   // (wave-uniform)
        const bool one_tile = __all(tc[0] == tc[last]);
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        for (int64_t r = ra; r < rb;) {
            // rows [r, re) of the segment lie in tile row ti
            const int64_t ti = (trow_off + r) / tile_rows;
            int64_t re = (ti + 1) * tile_rows - trow_off;
            re = re < rb ? re : rb;
            const int n = (int)(re - r);
            const uint8_t *p = buf + (r0 + r) * pitch_bytes + q * U::BYTES;
            // four rows' loads are issued before the first is used (digest_kernel); a row
            // past the tile row's last is the last row again and is not counted
            for (int j0 = 0; j0 < n; j0 += 4) {
                uint4 x[4][U::WORDS / 4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u < n ? j0 + u : n - 1;
#pragma unroll
                    for (int v = 0; v < U::WORDS / 4; ++v)
                        x[u][v] = reinterpret_cast<const uint4 *>(p + j * pitch_bytes)[v];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j0 + u >= n) break;   // (wave-uniform)
                    uint32_t w[U::WORDS];
#pragma unroll
                    for (int v = 0; v < U::WORDS / 4; ++v) {
                        w[4 * v] = x[u][v].x;
                        w[4 * v + 1] = x[u][v].y;
                        w[4 * v + 2] = x[u][v].z;
                        w[4 * v + 3] = x[u][v].w;
                    }
                    if (whole) acc[0] += on ? density_unit_whole<G>(w) : 0u;
                    else density_unit<G>(w, mask, h.s, acc);
                }
            }
            // flush the tile row's counts (a count that is not 0 has a cell of the window
            // in it, so its tile is inside the part; the range tests only repeat that)
            const int64_t tr = ti - ti_base;
            uint32_t *const prow = part + tr * tcols;
            const bool tr_ok = tr >= 0 && tr < ntr;
            if (one_tile) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t <= NL; ++t) v += acc[t];
                const int key = (int)tc[0];
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t ov = __shfl_down(v, off, 64);
                    const int ok = __shfl_down(key, off, 64);
                    if (lane + off < 64 && ok == key) v += ov;
                }
                const int before = __shfl_up(key, 1, 64);
                if ((lane == 0 || before != key) && v && tr_ok && key >= 0 && key < tcols) atomicAdd(prow + key, v);
            } else {
                uint32_t v = acc[0];
                int64_t key = tc[0];
#pragma unroll
                for (int t = 1; t <= NL; ++t) {
                    if (tc[t] == key) {
                        v += acc[t];
                    } else {
                        if (v && tr_ok && key >= 0 && key < tcols) atomicAdd(prow + key, v);
                        key = tc[t];
                        v = acc[t];
                    }
                }
                if (v && tr_ok && key >= 0 && key < tcols) atomicAdd(prow + key, v);
            }
#pragma unroll
            for (int t = 0; t <= NL; ++t) acc[t] = 0u;
            r = re;
        }
    }
}

hipError_t launch_density(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t trow_off, int64_t pc0,
                          int64_t lc0, int64_t ncols, int64_t col0, int64_t tile_rows, int64_t tile_cols,
                          uint32_t *part, int64_t ti_base, int64_t ntr, int64_t tcols, int bit_gw, hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    if (r0 < 0 || pc0 < 0 || col0 < 0 || lc0 < col0 || trow_off < 0 || tile_rows < 1 || tile_cols < 32 ||
        tile_cols % 32 || col0 % 32 || (bit_gw != 0 && bit_gw != 2 && bit_gw != 4))
        return hipErrorInvalidValue;
    // every tile the run touches lies inside the part
    if (trow_off / tile_rows < ti_base || (trow_off + nrows - 1) / tile_rows - ti_base >= ntr ||
        (lc0 + ncols - 1 - col0) / tile_cols >= tcols || tcols > INT32_MAX)
        return hipErrorInvalidValue;
    const int64_t ucols = bit_gw ? DigestUnit<2>::COLS : DigestUnit<0>::COLS;
    const int64_t q0 = pc0 / ucols, nunits = (pc0 + ncols - 1) / ucols - q0 + 1;
    const int64_t ncb = (nunits + 63) / 64;
    // segments of 64·m rows, chosen as launch_digest chooses them (tile rows cut them further)
    constexpr int64_t kMaxBlocks = 4096;
    int64_t m = (nrows + 63) / 64 * ncb / (kMaxBlocks * 4);
    m = m < 1 ? 1 : m > 8 ? 8 : m;
    int seg_rows = (int)(64 * m);
    const int64_t items = ncb * ((nrows + seg_rows - 1) / seg_rows);
    int64_t blocks = (items + 3) / 4;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const auto fn = bit_gw == 4 ? density_kernel<4> : bit_gw == 2 ? density_kernel<2> : density_kernel<0>;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint8_t *>(buf), pitch_bytes, r0,
                       nrows, trow_off, pc0, lc0, ncols, col0, tile_rows, tile_cols, seg_rows, q0, nunits, part, ti_base,
                       ntr, tcols);
    return hipGetLastError();
}

// ---------------------------------------------------------------- compiled rules
// The rules of GOL_COMPILED_RULES (gol_rule.h) on kernels of their own:
// bit_rule_kernel's body with the rule as template arguments, so the stage is
// rule_const_bits' immediates: no fifth argument, no table, no coefficient
// SGPRs.  Rings, chains and waves per depth are bit_rule_fn's.  Emitted behind
// every other kernel so that none of them moves.
template <uint32_t BIRTH, uint32_t SURVIVE>
struct ConstRuleStage {
    template <bool EDGE>
    __device__ __forceinline__ uint32_t apply(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0,
                                              uint32_t c1, uint32_t alive, uint32_t mask) const {
        return rule_const_bits<BIRTH, SURVIVE, EDGE>(a0, a1, b0, b1, c0, c1, alive, mask);
    }
};

template <int K, int NCH, int RING, int WPE, uint32_t BIRTH, uint32_t SURVIVE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE)))
void bit_crule_kernel(StencilArgs a, Sched q, int nstrips, int nblocks) {
    constexpr int V = 2, G = 2;
    for_each_item(a, q, nstrips, nblocks, [&](int strip, int r0, int r1) {
        Strip<V> st;
        st.setup(a, K, strip, r0, r1, 0u);
        const ConstRuleStage<BIRTH, SURVIVE> stage;
        constexpr int CL = (K + NCH - 1) / NCH;
        constexpr int M = 2 * K + (K - 1) / CL;   // as bit_pipe_kernel: the chunk's light cone
        const uint32_t all = st.mask[0] & st.mask[1];
        const bool full = __builtin_amdgcn_ballot_w64(all != 0xffffffffu) == 0ull;
        if (full && st.R0 - M >= a.row_lo && st.R1 + M <= a.row_hi) bit_run<V, K, CL, RING, 0, false, G>(st, a, stage);
        else bit_run<V, K, CL, RING, 0, true, G>(st, a, stage);
    });
}

template <uint32_t BIRTH, uint32_t SURVIVE>
static const void *bit_crule_fn_of(int gens) {
    switch (gens) {
    case 1: return (const void *)&bit_crule_kernel<1, 1, 18, 4, BIRTH, SURVIVE>;
    case 2: return (const void *)&bit_crule_kernel<2, 1, 24, 4, BIRTH, SURVIVE>;
    case 3: return (const void *)&bit_crule_kernel<3, 1, 6, 4, BIRTH, SURVIVE>;
    case 4: return (const void *)&bit_crule_kernel<4, 1, 6, 4, BIRTH, SURVIVE>;
    case 5: return (const void *)&bit_crule_kernel<5, 2, 6, 4, BIRTH, SURVIVE>;
    case 6: return (const void *)&bit_crule_kernel<6, 2, 6, 4, BIRTH, SURVIVE>;
    case 7: return (const void *)&bit_crule_kernel<7, 2, 6, 4, BIRTH, SURVIVE>;
    default: return nullptr;
    }
}

static const void *bit_crule_fn(int gens, int rule_index) {
    using Fn = const void *(*)(int);
#define GOL_CRULE_FN(name, b, s) &bit_crule_fn_of<rule_mask(b), rule_mask(s)>,
    static const Fn table[] = {GOL_COMPILED_RULES(GOL_CRULE_FN)};
#undef GOL_CRULE_FN
    static_assert(sizeof(table) / sizeof(table[0]) == kCompiledRuleCount, "one entry per listed rule");
    return rule_index >= 0 && rule_index < kCompiledRuleCount ? table[rule_index](gens) : nullptr;
}

bool bit_crule_supported(int gens, int gw, int rule_index) {
    return gw == 2 && bit_crule_fn(gens, rule_index) != nullptr;
}

hipError_t launch_bit_crule(const StencilArgs &a, int gens, int rule_index, hipStream_t s) {
    if (a.out_r1 <= a.out_r0) return hipSuccess;
    const void *fn = a.gw == 2 ? bit_crule_fn(gens, rule_index) : nullptr;
    if (!fn) return hipErrorInvalidValue;   // no fall-back: the caller asks bit_crule_supported first
    int waves = 0, ns = 0;
    Sched q = plan_items(a, gens, 2, true, fn, waves, ns);
    if (q.nitems <= 0) return hipSuccess;
    int nb = (waves + 3) / 4;
    StencilArgs aa = a;
    void *args[] = {&aa, &q, &ns, &nb};
    return hipLaunchKernel(fn, dim3(nb), dim3(256), args, 0, s);
}

} // namespace gol
