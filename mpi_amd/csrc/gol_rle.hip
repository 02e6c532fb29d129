// RLE pattern text on the device (gol_format_rle / gol_write_rle / gol_rle_bytes):
// packed rows (launch_get_bits' staging, gol_bits.h) -> the token stream of
// gol_rle.h, which holds the format and every per-lane routine, proven on the host
// by tests/fake_hip/rle_check.cpp.  A translation unit of its own, as gol_text.hip
// and gol_bits.hip are: no tuned kernel of gol_kernels.hip moves.
//
// Three launches per block of rows; no workgroup waits for another inside a launch
// (no look-back, no grid barrier, no polling): the launch boundaries hand over.
//   rle_rows_kernel   a workgroup per row (grid-stride): passes of 256 lanes x 4 words =
//                     32768 positions; a lane's last transition goes through an exclusive
//                     max-scan (prev of the lane's first token), its tokens and bytes are
//                     summed; between passes the workgroup carries the last transition and
//                     the sums.  Out: tokens and bytes (no newlines) per row.
//   rle_scan_kernel   ONE workgroup, 256 rows per pass: max-scan of the non-empty rows
//                     (the row before), then sums of tokens and bytes; carry-in from the
//                     host (last non-empty row, token index).  Out per row: `$` count,
//                     first token index, byte offset; the block's record.
//   rle_write_kernel  rle_rows_kernel's traversal with exclusive sums: every lane stores its
//                     tokens at the row's offset + its byte prefix + the newlines before its
//                     first token index; the lane of a row's first token stores the row's
//                     `$` token too.  Byte stores in plain C++.
// The scans use barriers inside one workgroup only.
#include "gol_internal.h"
#include "gol_rle.h"

namespace gol {

namespace {

struct MaxOp {
    __device__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};
struct SumOp {
    __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; }
};

// Exclusive scan of v over the workgroup's 256 lanes (4 waves), identity `ident`; *total = all of it.
// Every lane of the workgroup calls it (two barriers); lds holds 4 values.
template <typename Op>
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t ident, Op op, int64_t *lds, int64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = op(inc, o);
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int64_t base = ident, all = ident;
#pragma unroll
    for (int w = 0; w < kRleLanes / 64; ++w) {
        const int64_t x = lds[w];
        if (w < wave) base = op(base, x);
        all = op(all, x);
    }
    __syncthreads();   // lds is free for the next scan
    int64_t ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = ident;
    *total = all;
    return op(base, ex);
}

__global__ __launch_bounds__(kRleLanes) void rle_rows_kernel(const uint32_t *__restrict__ packed, int64_t pitch_words,
                                                             int64_t nrows, int64_t ncols, uint32_t *__restrict__ ntok,
                                                             uint32_t *__restrict__ nraw) {
    __shared__ int64_t lds[kRleLanes / 64];
    const int64_t spans = rle_row_spans(ncols);
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const uint32_t *row = packed + r * pitch_words;
        int64_t prev0 = 0, tok = 0, raw = 0;   // carries between passes (workgroup-uniform)
        for (int64_t g0 = 0; g0 < spans; g0 += kRleLanes) {
            const int64_t g = g0 + threadIdx.x;
            const RleSpan s = rle_span_load(row, g * kRleSpanWords, ncols);   // (past the row: no cells, no transitions)
            int64_t last_all, n_all, b_all, dn, db;
            int64_t prev = block_scan(rle_span_last(s), (int64_t)-1, MaxOp(), lds, &last_all);
            if (prev < prev0) prev = prev0;
            rle_span_count(s, prev, &dn, &db);
            block_scan(dn, (int64_t)0, SumOp(), lds, &n_all);
            block_scan(db, (int64_t)0, SumOp(), lds, &b_all);
            tok += n_all;
            raw += b_all;
            if (last_all > prev0) prev0 = last_all;
        }
        if (threadIdx.x == 0) {
            ntok[r] = (uint32_t)tok;
            nraw[r] = (uint32_t)raw;
        }
    }
}

__global__ __launch_bounds__(kRleLanes) void rle_scan_kernel(const uint32_t *__restrict__ ntok,
                                                             const uint32_t *__restrict__ nraw, int64_t nrows,
                                                             int64_t row_base, int64_t last_row, int64_t tok0, int L,
                                                             uint32_t *__restrict__ dcount, int64_t *__restrict__ tix,
                                                             int64_t *__restrict__ off, RleRecord *__restrict__ rec) {
    __shared__ int64_t lds[kRleLanes / 64];
    int64_t tok = tok0, raw = 0;   // carries between passes (workgroup-uniform), last_row too
    for (int64_t r0 = 0; r0 < nrows; r0 += kRleLanes) {
        const int64_t r = r0 + threadIdx.x;
        const bool on = r < nrows;
        const int64_t n = on ? ntok[r] : 0, b = on ? nraw[r] : 0;
        int64_t last_all, n_all, b_all;
        int64_t before = block_scan(n ? row_base + r : (int64_t)-1, (int64_t)-1, MaxOp(), lds, &last_all);
        if (before < last_row) before = last_row;
        const RleRowHead h = rle_row_head(row_base + r, before, n, b);
        const int64_t t = tok + block_scan(h.tokens, (int64_t)0, SumOp(), lds, &n_all);
        const int64_t o = raw + block_scan(h.raw, (int64_t)0, SumOp(), lds, &b_all);
        if (on) {
            dcount[r] = (uint32_t)h.dcount;
            tix[r] = t;
            off[r] = o + rle_newlines(tok0, t - tok0, L);
        }
        tok += n_all;
        raw += b_all;
        if (last_all > last_row) last_row = last_all;
    }
    if (threadIdx.x == 0) {
        rec->bytes = raw + rle_newlines(tok0, tok - tok0, L);
        rec->tokens = tok;
        rec->last_row = last_row;
    }
}

__global__ __launch_bounds__(kRleLanes) void rle_write_kernel(const uint32_t *__restrict__ packed, int64_t pitch_words,
                                                              int64_t nrows, int64_t ncols,
                                                              const uint32_t *__restrict__ ntok,
                                                              const uint32_t *__restrict__ dcount,
                                                              const int64_t *__restrict__ tix,
                                                              const int64_t *__restrict__ off, int L,
                                                              char *__restrict__ text) {
    __shared__ int64_t lds[kRleLanes / 64];
    const int64_t spans = rle_row_spans(ncols);
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        if (!ntok[r]) continue;   // (workgroup-uniform) an empty row has no byte of its own
        const uint32_t *row = packed + r * pitch_words;
        char *base = text + off[r];
        const uint32_t dc = dcount[r], uL = (uint32_t)L;
        const uint32_t m0 = (uint32_t)(tix[r] % L);   // the row's first token index mod L
        // behind the row's `$` token: the first run token's index in the row and its byte
        const uint32_t j0 = dc > 0;
        const int raw0 = dc ? rle_token_bytes(dc) : 0;
        int64_t prev0 = 0, tok = 0, raw = 0;
        for (int64_t q0 = 0; q0 < spans; q0 += kRleLanes) {
            const int64_t q = q0 + threadIdx.x;
            const RleSpan s = rle_span_load(row, q * kRleSpanWords, ncols);
            int64_t last_all, n_all, b_all, dn, db;
            int64_t prev = block_scan(rle_span_last(s), (int64_t)-1, MaxOp(), lds, &last_all);
            if (prev < prev0) prev = prev0;
            rle_span_count(s, prev, &dn, &db);
            const int64_t j = tok + block_scan(dn, (int64_t)0, SumOp(), lds, &n_all);
            const int64_t at = raw + block_scan(db, (int64_t)0, SumOp(), lds, &b_all);
            if (dn) {
                if (j == 0 && dc) rle_put_token(base, dc, '$', m0 == uL - 1);
                const uint32_t g = m0 + j0 + (uint32_t)j;   // (a row has at most 2^31 + 1 tokens)
                rle_span_write(s, prev, (int)(g % uL), L, base + raw0 + at + g / uL);
            }
            tok += n_all;
            raw += b_all;
            if (last_all > prev0) prev0 = last_all;
        }
    }
}

unsigned row_grid(int64_t nrows) { return (unsigned)(nrows < 65536 ? nrows : 65536); }

} // namespace

hipError_t launch_rle_rows(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols, uint32_t *ntok,
                           uint32_t *nraw, hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    if (!packed || !ntok || !nraw || ncols < 1 || (ncols + 31) / 32 > pitch_words) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rle_rows_kernel, dim3(row_grid(nrows)), dim3(kRleLanes), 0, s, packed, pitch_words, nrows, ncols,
                       ntok, nraw);
    return hipGetLastError();
}

hipError_t launch_rle_scan(const uint32_t *ntok, const uint32_t *nraw, int64_t nrows, int64_t row_base,
                           int64_t last_row, int64_t tok0, int L, uint32_t *dcount, int64_t *tix, int64_t *off,
                           RleRecord *rec, hipStream_t s) {
    if (!ntok || !nraw || !dcount || !tix || !off || !rec || nrows < 0 || L < 1 || tok0 < 0 || last_row >= row_base)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(kRleLanes), 0, s, ntok, nraw, nrows, row_base, last_row, tok0, L,
                       dcount, tix, off, rec);
    return hipGetLastError();
}

hipError_t launch_rle_write(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols,
                            const uint32_t *ntok, const uint32_t *dcount, const int64_t *tix, const int64_t *off, int L,
                            char *text, hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    if (!packed || !ntok || !dcount || !tix || !off || !text || ncols < 1 || L < 1 || (ncols + 31) / 32 > pitch_words)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rle_write_kernel, dim3(row_grid(nrows)), dim3(kRleLanes), 0, s, packed, pitch_words, nrows, ncols,
                       ntok, dcount, tix, off, L, text);
    return hipGetLastError();
}

} // namespace gol
