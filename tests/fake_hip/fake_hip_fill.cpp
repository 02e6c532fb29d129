// Host-only stand-in for the random-fill launcher (test infrastructure, the
// companion of fake_hip.cpp and fake_hip_bits.cpp: see their headers).  It
// computes: the stand-in's "device" memory is host memory, so the row routine of
// gol_fill.h runs here directly and the CPU suite checks the runtime's side of
// gol_fill_random* — slabs and seams, windows, column runs, the torus margin, the
// inactive cells, rank contexts — on byte-layout boards, whose byte downloads are
// plain copies (tests/fill_cpu_check.py), beside the recorded schedule
// (tests/sched_fill_check.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_fill.h"
#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {

hipError_t launch_fill_random(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                              int64_t lc0, int64_t ncols, int64_t active_cols, uint64_t K, uint64_t T, int bit_gw,
                              hipStream_t) {
    if (r1 <= r0 || ncols <= 0) return hipSuccess;
    if (r0 < 0 || pc0 < 0 || lc0 < 0 || grow0 < 0 || T > kFillFull || !(bit_gw == 0 || bit_gw == 2 || bit_gw == 4))
        return hipErrorInvalidValue;
    uint8_t *b = static_cast<uint8_t *>(buf);
    for (int64_t r = r0; r < r1; ++r) {
        uint8_t *row = b + r * pitch_bytes;
        const int64_t g = grow0 + (r - r0);
        if (bit_gw == 4) fill_put_row<4>(row, pc0, lc0, ncols, active_cols, K, T, g);
        else if (bit_gw == 2) fill_put_row<2>(row, pc0, lc0, ncols, active_cols, K, T, g);
        else fill_put_row<0>(row, pc0, lc0, ncols, active_cols, K, T, g);
    }
    return hipSuccess;
}
}  // namespace gol
