// Host-only stand-in for the RLE launchers (test infrastructure, the companion of
// fake_hip.cpp and fake_hip_bits.cpp: see their headers).  It computes: the three
// passes of gol_rle.h run on the stand-in's host "device" memory lane after lane,
// so the CPU suite checks the runtime's side of gol_format_rle / gol_write_rle /
// gol_rle_bytes / gol_parse_rle — blocks, slab pieces, the carries between them,
// the exact-size copies — against tests/rle_ref.py (tests/rle_cpu_check.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_internal.h"
#include "../../mpi_amd/csrc/gol_rle.h"

namespace gol {

hipError_t launch_rle_rows(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols, uint32_t *ntok,
                           uint32_t *nraw, hipStream_t) {
    if (nrows <= 0) return hipSuccess;
    if (!packed || !ntok || !nraw || ncols < 1 || (ncols + 31) / 32 > pitch_words) return hipErrorInvalidValue;
    rle_row_pass_host(packed, pitch_words, nrows, ncols, ntok, nraw);
    return hipSuccess;
}

hipError_t launch_rle_scan(const uint32_t *ntok, const uint32_t *nraw, int64_t nrows, int64_t row_base,
                           int64_t last_row, int64_t tok0, int L, uint32_t *dcount, int64_t *tix, int64_t *off,
                           RleRecord *rec, hipStream_t) {
    if (!ntok || !nraw || !dcount || !tix || !off || !rec || nrows < 0 || L < 1 || tok0 < 0 || last_row >= row_base)
        return hipErrorInvalidValue;
    rle_row_scan_host(ntok, nraw, nrows, row_base, last_row, tok0, L, dcount, tix, off, rec);
    return hipSuccess;
}

hipError_t launch_rle_write(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols,
                            const uint32_t *ntok, const uint32_t *dcount, const int64_t *tix, const int64_t *off, int L,
                            char *text, hipStream_t) {
    if (nrows <= 0) return hipSuccess;
    if (!packed || !ntok || !dcount || !tix || !off || !text || ncols < 1 || L < 1 || (ncols + 31) / 32 > pitch_words)
        return hipErrorInvalidValue;
    rle_write_pass_host(packed, pitch_words, nrows, ncols, ntok, dcount, tix, off, L, text);
    return hipSuccess;
}

}  // namespace gol
