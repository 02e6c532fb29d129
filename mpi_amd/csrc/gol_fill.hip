// The counter-based random fill on the device (gol_fill_random*): gol_fill.h holds
// the definition and the per-unit routines, proven on the host by
// tests/fake_hip/fill_check.cpp.  A translation unit of its own, as gol_bits.hip
// is: no tuned kernel of gol_kernels.hip moves.
//
// put_bits_kernel's streaming shape: a wave takes items of 64 units along the row
// (a lane = one unit: 16 B of a bit row, 32 B of a byte row) times a segment of
// 64·m rows; per item a lane computes its merge masks, its shift and its global
// word index once and keeps them down the rows.  Per row: one row key sm(K + r),
// wave-uniform (scalar unit); the plane hashes of the lane's NL (+1 when the column
// shift is non-zero) canonical words, from the first hash the threshold needs
// (launch-uniform, so the loop and the threshold's bits are scalar control); the
// merge; one 16-byte store per 4 storage words.  A unit is read only when the run
// does not cover it (window edges, a partial last unit): a whole-board fill of
// interior units is write-only.  No other lane touches the unit, so no atomics.
#include "gol_fill.h"
#include "gol_internal.h"

namespace gol {

namespace {

template <int G>
__global__ __launch_bounds__(256) void fill_random_kernel(uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                                          int64_t nrows, int64_t grow0, int64_t pc0, int64_t lc0,
                                                          int64_t ncols, int64_t active_cols, int seg_rows, int64_t q0,
                                                          int64_t nunits, uint64_t K, uint32_t T, int j0,
                                                          uint32_t constant) {
    typedef DigestUnit<G> U;
    constexpr int NL = U::NL, W = U::WORDS;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    const bool carry = ((lc0 - pc0) & 31) != 0;   // launch-uniform: canonical word NL reaches the unit
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        if (cb * 64 + lane >= nunits) continue;   // units are a lane's own: nothing is shared with the idle lanes
        const int64_t q = q0 + cb * 64 + lane;
        const BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc0, ncols);
        const BitsPutMask<G> m = bits_put_mask_of<G>(q, u, active_cols);
        bool covered = true;   // the run replaces every cell of the unit: nothing to read
#pragma unroll
        for (int k = 0; k < W; ++k) covered = covered && m.keep[k] == 0xffffffffu;
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        uint8_t *p = buf + (r0 + ra) * pitch_bytes + q * U::BYTES;
        const uint64_t wbase = 16u * (uint64_t)u.w0;
        for (int64_t i0 = 0; i0 < rb - ra; i0 += 4) {
            uint32_t x[4][W];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int v = 0; v < W; ++v) x[k][v] = 0u;
            }
            if (!covered) {   // four rows' loads issued before the first is used
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t i = i0 + k < rb - ra ? i0 + k : rb - ra - 1;
                    const uint4 *s = reinterpret_cast<const uint4 *>(p + i * pitch_bytes);
#pragma unroll
                    for (int v = 0; v < W / 4; ++v) {
                        const uint4 y = s[v];
                        x[k][4 * v] = y.x;
                        x[k][4 * v + 1] = y.y;
                        x[k][4 * v + 2] = y.z;
                        x[k][4 * v + 3] = y.w;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k >= rb - ra) continue;   // (wave-uniform)
                uint32_t C[NL + 1];
#pragma unroll
                for (int t = 0; t <= NL; ++t) C[t] = constant;   // T = 0 or 2^32 (j0 = 16): no hash
                if (j0 < 16) {
                    const uint64_t base = fill_row_key(K, grow0 + ra + i0 + k) + wbase;   // row key: wave-uniform
#pragma unroll
                    for (int t = 0; t <= NL; ++t) C[t] = 0u;
                    for (int j = j0; j < 16; ++j) {
                        const uint32_t mlo = 0u - ((T >> (2 * j)) & 1u), mhi = 0u - ((T >> (2 * j + 1)) & 1u);
#pragma unroll
                        for (int t = 0; t < NL; ++t) {
                            const uint64_t h = digest_sm(base + (uint64_t)(16 * t + j));
                            C[t] = fill_plane(fill_plane(C[t], (uint32_t)h, mlo), (uint32_t)(h >> 32), mhi);
                        }
                        if (carry) {
                            const uint64_t h = digest_sm(base + (uint64_t)(16 * NL + j));
                            C[NL] = fill_plane(fill_plane(C[NL], (uint32_t)h, mlo), (uint32_t)(h >> 32), mhi);
                        }
                    }
                }
                fill_put_unit<G>(x[k], u, m, C);
                uint4 *d = reinterpret_cast<uint4 *>(p + (i0 + k) * pitch_bytes);
#pragma unroll
                for (int v = 0; v < W / 4; ++v)
                    d[v] = make_uint4(x[k][4 * v], x[k][4 * v + 1], x[k][4 * v + 2], x[k][4 * v + 3]);
            }
        }
    }
}

}  // namespace

// items and grid as bits_grid (gol_bits.hip) chooses them
hipError_t launch_fill_random(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                              int64_t lc0, int64_t ncols, int64_t active_cols, uint64_t K, uint64_t T, int bit_gw,
                              hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    if (r0 < 0 || pc0 < 0 || lc0 < 0 || grow0 < 0 || T > kFillFull || !(bit_gw == 0 || bit_gw == 2 || bit_gw == 4))
        return hipErrorInvalidValue;
    const int64_t ucols = bit_gw ? DigestUnit<2>::COLS : DigestUnit<0>::COLS;
    const int64_t q0 = pc0 / ucols, nunits = (pc0 + ncols - 1) / ucols - q0 + 1;
    const int64_t ncb = (nunits + 63) / 64;
    constexpr int64_t kMaxBlocks = 4096;
    int64_t m = (nrows + 63) / 64 * ncb / (kMaxBlocks * 4);
    m = m < 1 ? 1 : m > 8 ? 8 : m;
    const int seg_rows = (int)(64 * m);
    const int64_t items = ncb * ((nrows + seg_rows - 1) / seg_rows);
    const int64_t blocks = (items + 3) / 4 > kMaxBlocks ? kMaxBlocks : (items + 3) / 4;
    const auto fn = bit_gw == 4 ? fill_random_kernel<4> : bit_gw == 2 ? fill_random_kernel<2> : fill_random_kernel<0>;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<uint8_t *>(buf), pitch_bytes, r0, nrows,
                       grow0, pc0, lc0, ncols, active_cols, seg_rows, q0, nunits, K, (uint32_t)T, fill_first_hash(T),
                       T ? 0xffffffffu : 0u);
    return hipGetLastError();
}

}  // namespace gol
