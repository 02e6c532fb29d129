// 1-bit-per-cell board I/O on the device (gol_download_bits* / gol_upload_bits*):
// storage rows of every layout <-> packed rows, MSB first (gol_bits.h holds the
// format and the per-unit routines, proven on the host by
// tests/fake_hip/bits_check.cpp).  A translation unit of its own, as gol_text.hip
// is: no tuned kernel of gol_kernels.hip moves.
//
// Both kernels have digest_kernel's streaming shape: a wave takes items of 64
// units along the row (a lane = one unit: 16 B of a bit row, 32 B of a byte row)
// times a segment of 64·m rows; per item a lane computes its window masks, its
// shift and its packed word index once and keeps them down the rows; four rows'
// loads are issued before the first is used.
//
// get: unit q yields NL + 1 packed words at words w0 .. w0 + NL of the packed
// row, w0(q + 1) = w0(q) + NL: a lane's top word (the carry of the column shift
// s) and its right neighbour's word 0 are one word, so it moves one lane up
// (__shfl_up) and every lane stores its words 0 .. NL - 1, each exactly once.
// Lanes past the run's last unit load the first unit under a zero mask, keep
// their own word index and so store the last unit's carry.  Three kinds of word
// are OR-ed (vector atomicOr into the cleared staging row) rather than stored:
// word 0 of lane 0 and the carry of lane 63, which meet between two items, and
// the first and last word of the run, which other runs of the same window may
// share (MESH_COMPAT).  Words outside the run's [first, last] hold no cell of
// the run and are not written.
//
// put: a lane reads the NL + 1 packed words of its unit itself (neighbours
// overlap by one word, served by the cache) and merges them into its own unit
// under masks computed once: no other lane touches the unit, so no atomics.
#include "gol_bits.h"
#include "gol_internal.h"

namespace gol {

namespace {

struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t v[4];   // a 16-byte store at dword alignment (the packed word index is arbitrary)
};

template <int G>
__device__ __forceinline__ void load_unit(const uint8_t *p, uint32_t *w) {
#pragma unroll
    for (int v = 0; v < DigestUnit<G>::WORDS / 4; ++v) {
        const uint4 x = reinterpret_cast<const uint4 *>(p)[v];
        w[4 * v] = x.x;
        w[4 * v + 1] = x.y;
        w[4 * v + 2] = x.z;
        w[4 * v + 3] = x.w;
    }
}

template <int G>
__global__ __launch_bounds__(256) void get_bits_kernel(const uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                                       int64_t nrows, int64_t pc0, int64_t lc0, int64_t ncols,
                                                       int seg_rows, int64_t q0, int64_t nunits,
                                                       uint32_t *__restrict__ out, int64_t opitch) {
    typedef DigestUnit<G> U;
    constexpr int NL = U::NL;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    const int64_t lo = bits_first_word(lc0), hi = bits_last_word(lc0, ncols);
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        const bool on = cb * 64 + lane < nunits;
        const int64_t q = q0 + cb * 64 + lane;
        BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc0, ncols);
        if (!on) {
#pragma unroll
            for (int t = 0; t < NL; ++t) u.mask[t] = 0u;
        }
        // per word t < NL: 0 = not written, 1 = stored, 2 = OR-ed; `top`: lane 63's carry is OR-ed
        int kind[NL];
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            const int64_t i = u.w0 + t;
            kind[t] = i < lo || i > hi ? 0 : (i == lo || i == hi || (t == 0 && lane == 0)) ? 2 : 1;
        }
        const bool top = lane == 63 && u.w0 + NL >= lo && u.w0 + NL <= hi;
        bool wide = NL == 4;
#pragma unroll
        for (int t = 0; t < NL; ++t) wide = wide && kind[t] == 1;
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        const uint8_t *p = buf + (r0 + ra) * pitch_bytes + (on ? q : q0) * U::BYTES;
        uint32_t *o = out + ra * opitch + u.w0;
        // the next four rows' loads are issued BEFORE this block's stores: loads and stores
        // return in order (one vmcnt), so a load issued behind a store waits for the store too
        const int64_t nr = rb - ra;
        uint32_t x[4][U::WORDS], nx[4][U::WORDS];
#pragma unroll
        for (int k = 0; k < 4; ++k) load_unit<G>(p + (k < nr ? k : nr - 1) * pitch_bytes, x[k]);
        for (int64_t j0 = 0; j0 < nr; j0 += 4) {
            if (j0 + 4 < nr) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t j = j0 + 4 + k < nr ? j0 + 4 + k : nr - 1;   // past the last row: it again, not stored
                    load_unit<G>(p + j * pitch_bytes, nx[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t P[NL + 1];
                bits_get_unit<G>(x[k], u, P);
                const uint32_t carry = __shfl_up(P[NL], 1, 64);
                if (lane > 0) P[0] |= carry;
                if (j0 + k >= nr) continue;   // (wave-uniform)
                uint32_t *d = o + (j0 + k) * opitch;
                if (wide) {
                    if constexpr (NL == 4) {
                        Words4 v;
#pragma unroll
                        for (int t = 0; t < 4; ++t) v.v[t] = P[t];
                        *reinterpret_cast<Words4 *>(d) = v;
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NL; ++t) {
                        if (kind[t] == 1) d[t] = P[t];
                        else if (kind[t] == 2 && P[t]) atomicOr(d + t, P[t]);
                    }
                }
                if (top && P[NL]) atomicOr(d + NL, P[NL]);
            }
            if (j0 + 4 < nr) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int v = 0; v < U::WORDS; ++v) x[k][v] = nx[k][v];
            }
        }
    }
}

template <int G>
__global__ __launch_bounds__(256) void put_bits_kernel(uint8_t *__restrict__ buf, int64_t pitch_bytes, int64_t r0,
                                                       int64_t nrows, int64_t pc0, int64_t lc0, int64_t ncols,
                                                       int64_t active_cols, int seg_rows, int64_t q0, int64_t nunits,
                                                       const uint32_t *__restrict__ in, int64_t ipitch) {
    typedef DigestUnit<G> U;
    constexpr int NL = U::NL;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ncb = (nunits + 63) / 64, nseg = (nrows + seg_rows - 1) / seg_rows;
    const int64_t lo = bits_first_word(lc0), hi = bits_last_word(lc0, ncols);
    for (int64_t item = wave; item < ncb * nseg; item += nwaves) {
        const int64_t seg = item / ncb, cb = item % ncb;
        if (cb * 64 + lane >= nunits) continue;   // units are a lane's own: nothing is shared with the idle lanes
        const int64_t q = q0 + cb * 64 + lane;
        const BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc0, ncols);
        const BitsPutMask<G> m = bits_put_mask_of<G>(q, u, active_cols);
        bool have[NL + 1];   // packed words outside the run's are not read (they hold none of its cells)
#pragma unroll
        for (int t = 0; t <= NL; ++t) have[t] = u.w0 + t >= lo && u.w0 + t <= hi;
        const int64_t ra = seg * seg_rows, rb = ra + seg_rows < nrows ? ra + seg_rows : nrows;
        uint8_t *p = buf + (r0 + ra) * pitch_bytes + q * U::BYTES;
        const uint32_t *src = in + ra * ipitch + u.w0;
        for (int64_t j0 = 0; j0 < rb - ra; j0 += 4) {
            uint32_t x[4][U::WORDS], P[4][NL + 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = j0 + k < rb - ra ? j0 + k : rb - ra - 1;
                load_unit<G>(p + j * pitch_bytes, x[k]);
#pragma unroll
                for (int t = 0; t <= NL; ++t) P[k][t] = have[t] ? src[j * ipitch + t] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (j0 + k >= rb - ra) continue;
                bits_put_unit<G>(x[k], u, m, P[k]);
                uint4 *d = reinterpret_cast<uint4 *>(p + (j0 + k) * pitch_bytes);
#pragma unroll
                for (int v = 0; v < U::WORDS / 4; ++v)
                    d[v] = make_uint4(x[k][4 * v], x[k][4 * v + 1], x[k][4 * v + 2], x[k][4 * v + 3]);
            }
        }
    }
}

// items and grid as launch_digest chooses them
struct BitsGrid {
    int64_t q0, nunits;
    int seg_rows;
    unsigned blocks;
};
BitsGrid bits_grid(int64_t nrows, int64_t pc0, int64_t ncols, int bit_gw) {
    const int64_t ucols = bit_gw ? DigestUnit<2>::COLS : DigestUnit<0>::COLS;
    BitsGrid g;
    g.q0 = pc0 / ucols;
    g.nunits = (pc0 + ncols - 1) / ucols - g.q0 + 1;
    const int64_t ncb = (g.nunits + 63) / 64;
    constexpr int64_t kMaxBlocks = 4096;
    int64_t m = (nrows + 63) / 64 * ncb / (kMaxBlocks * 4);
    m = m < 1 ? 1 : m > 8 ? 8 : m;
    g.seg_rows = (int)(64 * m);
    const int64_t items = ncb * ((nrows + g.seg_rows - 1) / g.seg_rows);
    const int64_t blocks = (items + 3) / 4;
    g.blocks = (unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks);
    return g;
}

bool bits_args_ok(int64_t r0, int64_t pc0, int64_t lc0, int64_t ncols, const void *packed, int64_t pitch_words,
                  int bit_gw) {
    return r0 >= 0 && pc0 >= 0 && lc0 >= 0 && packed && (bit_gw == 0 || bit_gw == 2 || bit_gw == 4) &&
           bits_last_word(lc0, ncols) < pitch_words;   // every word a lane touches lies in the packed row
}

} // namespace

hipError_t launch_get_bits(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, uint32_t *out, int64_t out_pitch_words, int bit_gw, hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    if (!bits_args_ok(r0, pc0, lc0, ncols, out, out_pitch_words, bit_gw)) return hipErrorInvalidValue;
    const BitsGrid g = bits_grid(nrows, pc0, ncols, bit_gw);
    const auto fn = bit_gw == 4 ? get_bits_kernel<4> : bit_gw == 2 ? get_bits_kernel<2> : get_bits_kernel<0>;
    hipLaunchKernelGGL(fn, dim3(g.blocks), dim3(256), 0, s, static_cast<const uint8_t *>(buf), pitch_bytes, r0, nrows,
                       pc0, lc0, ncols, g.seg_rows, g.q0, g.nunits, out, out_pitch_words);
    return hipGetLastError();
}

hipError_t launch_put_bits(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, int64_t active_cols, const uint32_t *in, int64_t in_pitch_words, int bit_gw,
                           hipStream_t s) {
    const int64_t nrows = r1 - r0;
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    if (!bits_args_ok(r0, pc0, lc0, ncols, in, in_pitch_words, bit_gw)) return hipErrorInvalidValue;
    const BitsGrid g = bits_grid(nrows, pc0, ncols, bit_gw);
    const auto fn = bit_gw == 4 ? put_bits_kernel<4> : bit_gw == 2 ? put_bits_kernel<2> : put_bits_kernel<0>;
    hipLaunchKernelGGL(fn, dim3(g.blocks), dim3(256), 0, s, static_cast<uint8_t *>(buf), pitch_bytes, r0, nrows, pc0,
                       lc0, ncols, active_cols, g.seg_rows, g.q0, g.nunits, in, in_pitch_words);
    return hipGetLastError();
}

} // namespace gol
