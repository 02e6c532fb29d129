// Board-to-board copies on the device (gol_copy_window / gol_copy): gol_copy.h holds
// the definition and the per-unit routines, proven on the host by
// tests/fake_hip/copy_check.cpp.  A translation unit of its own, as gol_bits.hip and
// gol_fill.hip are: no tuned kernel of gol_kernels.hip moves.
//
// put_bits_kernel's streaming shape: a wave takes items of 64 DESTINATION units
// along the row (a lane = one unit: 16 B of a bit row, 32 B of a byte row) times a
// segment of 64·m rows; per item a lane computes its merge masks, its shift and its
// covering range of source units once and keeps them down the rows; the loads of
// kRows rows (the source units and, where needed, the destination unit) are issued
// before the first is used.  Every destination word is written by exactly one lane:
// no atomics, no carry between lanes.  A lane reads its MAXU covering source units
// whole (neighbouring lanes overlap by one unit, served by the cache), but only
// those of the source run's own units [first, last]: the others hold no cell of the
// run and may lie outside the allocation (CopyUnit::have).  A destination unit the
// run covers entirely is not read under REPLACE.
//
// src and dst may be one buffer (a window tiled within one board): they are not
// __restrict__, every row batch is loaded before its stores, and a merge changes no
// bit outside the destination run, so a source bit that shares a word with
// destination cells reads the same before and after the other lane's store.
#include "gol_copy.h"
#include "gol_internal.h"

namespace gol {

namespace {

template <int WORDS>
__device__ __forceinline__ void load_words(const uint8_t *p, uint32_t *w) {
#pragma unroll
    for (int v = 0; v < WORDS / 4; ++v) {
        const uint4 x = reinterpret_cast<const uint4 *>(p)[v];
        w[4 * v] = x.x;
        w[4 * v + 1] = x.y;
        w[4 * v + 2] = x.z;
        w[4 * v + 3] = x.w;
    }
}

// rows whose loads are in flight together: a byte source unit is 8 registers and a
// bit destination unit covers up to five of them
template <int GS, int GD> struct CopyRows {
    static constexpr int N = GS ? 4 : GD ? 1 : 2;
};

template <int GS, int GD>
__global__ __launch_bounds__(256) void copy_cells_kernel(const uint8_t *src, int64_t spitch, int64_t sr0, uint8_t *dst,
                                                         int64_t dpitch, int64_t dr0, int64_t nrows, int64_t spc0,
                                                         int64_t dpc0, int64_t ncols, int64_t active_cols, int op,
                                                         int seg_rows, int64_t q0, int64_t nunits) {
    typedef CopyPair<GS, GD> P;
    constexpr int kRows = CopyRows<GS, GD>::N;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        if (cb * 64 + lane >= nunits) continue;   // units are a lane's own: nothing is shared with the idle lanes
        const int64_t q = q0 + cb * 64 + lane;
        const CopyUnit<GS, GD> cu = copy_unit_of<GS, GD>(q, spc0, dpc0, ncols, active_cols);
        const bool read = !(cu.covered && op == kCopyReplace);
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        // (an offset, not a pointer: unit u0 may lie before the row; it is added only where have[k])
        const int64_t soff = (sr0 + ra) * spitch + cu.u0 * DigestUnit<GS>::BYTES;
        uint8_t *dp = dst + (dr0 + ra) * dpitch + q * DigestUnit<GD>::BYTES;
        const int64_t nr = rb - ra;
        for (int64_t i0 = 0; i0 < nr; i0 += kRows) {
            uint32_t xs[kRows][P::MAXU][P::WS], w[kRows][P::WD];
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int64_t i = i0 + k < nr ? i0 + k : nr - 1;   // past the last row: it again, not stored
#pragma unroll
                for (int u = 0; u < P::MAXU; ++u) {
#pragma unroll
                    for (int v = 0; v < P::WS; ++v) xs[k][u][v] = 0u;
                    if (cu.have[u]) load_words<P::WS>(src + soff + i * spitch + u * DigestUnit<GS>::BYTES, xs[k][u]);
                }
#pragma unroll
                for (int v = 0; v < P::WD; ++v) w[k][v] = 0u;
                if (read) load_words<P::WD>(dp + i * dpitch, w[k]);
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                if (i0 + k >= nr) continue;   // (wave-uniform)
                copy_unit<GS, GD>(xs[k], w[k], cu, op);
                uint4 *d = reinterpret_cast<uint4 *>(dp + (i0 + k) * dpitch);
#pragma unroll
                for (int v = 0; v < P::WD / 4; ++v)
                    d[v] = make_uint4(w[k][4 * v], w[k][4 * v + 1], w[k][4 * v + 2], w[k][4 * v + 3]);
            }
        }
    }
}

template <int GS, int GD>
void launch_pair(unsigned blocks, hipStream_t s, const uint8_t *src, int64_t spitch, int64_t sr0, uint8_t *dst,
                 int64_t dpitch, int64_t dr0, int64_t nrows, int64_t spc0, int64_t dpc0, int64_t ncols,
                 int64_t active_cols, int op, int seg_rows, int64_t q0, int64_t nunits) {
    hipLaunchKernelGGL((copy_cells_kernel<GS, GD>), dim3(blocks), dim3(256), 0, s, src, spitch, sr0, dst, dpitch, dr0,
                       nrows, spc0, dpc0, ncols, active_cols, op, seg_rows, q0, nunits);
}

}  // namespace

// items and grid as bits_grid (gol_bits.hip) chooses them, over the destination's units
hipError_t launch_copy_cells(const void *src, int64_t src_pitch_bytes, int64_t sr0, int64_t spc0, int src_gw, void *dst,
                             int64_t dst_pitch_bytes, int64_t dr0, int64_t dpc0, int dst_gw, int64_t nrows,
                             int64_t ncols, int64_t active_cols, int op, hipStream_t s) {
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    const auto gw_ok = [](int g) { return g == 0 || g == 2 || g == 4; };
    if (!src || !dst || sr0 < 0 || dr0 < 0 || spc0 < 0 || dpc0 < 0 || !gw_ok(src_gw) || !gw_ok(dst_gw) ||
        op < kCopyReplace || op > kCopyXor)
        return hipErrorInvalidValue;
    const int64_t ucols = dst_gw ? DigestUnit<2>::COLS : DigestUnit<0>::COLS;
    const int64_t q0 = dpc0 / ucols, nunits = (dpc0 + ncols - 1) / ucols - q0 + 1;
    const int64_t ncb = (nunits + 63) / 64;
    constexpr int64_t kMaxBlocks = 4096;
    int64_t m = (nrows + 63) / 64 * ncb / (kMaxBlocks * 4);
    m = m < 1 ? 1 : m > 8 ? 8 : m;
    const int seg_rows = (int)(64 * m);
    const int64_t items = ncb * ((nrows + seg_rows - 1) / seg_rows);
    const unsigned blocks = (unsigned)((items + 3) / 4 > kMaxBlocks ? kMaxBlocks : (items + 3) / 4);
    const uint8_t *sb = static_cast<const uint8_t *>(src);
    uint8_t *db = static_cast<uint8_t *>(dst);
#define GOL_COPY_PAIR(GS, GD)                                                                                        \
    if (src_gw == GS && dst_gw == GD)                                                                                \
        launch_pair<GS, GD>(blocks, s, sb, src_pitch_bytes, sr0, db, dst_pitch_bytes, dr0, nrows, spc0, dpc0, ncols, \
                            active_cols, op, seg_rows, q0, nunits);
    GOL_COPY_PAIR(0, 0)
    GOL_COPY_PAIR(0, 2)
    GOL_COPY_PAIR(0, 4)
    GOL_COPY_PAIR(2, 0)
    GOL_COPY_PAIR(2, 2)
    GOL_COPY_PAIR(2, 4)
    GOL_COPY_PAIR(4, 0)
    GOL_COPY_PAIR(4, 2)
    GOL_COPY_PAIR(4, 4)
#undef GOL_COPY_PAIR
    return hipGetLastError();
}

}  // namespace gol
