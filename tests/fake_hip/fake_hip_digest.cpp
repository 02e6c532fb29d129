// Host-only stand-in for the digest launcher (test infrastructure, the companion
// of fake_hip.cpp: see its header).  Unlike the stencil stand-ins it computes:
// the stand-in's "device" memory is host memory, so the row routine of
// gol_digest.h runs here directly and the CPU suite checks the runtime's side of
// gol_digest* — slabs, column runs, the torus margin, windows, the pending ring —
// on byte-layout boards, whose uploads and downloads are plain copies
// (tests/test_digest_cpu.py), beside the recorded schedule
// (tests/sched_digest_check.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_digest.h"
#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {
namespace {
template <int G>
void digest_rows(const uint8_t *buf, int64_t pitch, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0, int64_t lc0,
                 int64_t ncols, unsigned long long *slot) {
    for (int64_t r = r0; r < r1; ++r) {
        uint64_t sum[2];
        digest_row<G>(buf + r * pitch, pc0, lc0, ncols, sum);
        for (int i = 0; i < 2; ++i) slot[i] += digest_A(i, grow0 + (r - r0)) * sum[i];
    }
}
}  // namespace

hipError_t launch_digest(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t grow0, int64_t pc0,
                         int64_t lc0, int64_t ncols, unsigned long long *slot, int bit_gw, hipStream_t) {
    const uint8_t *b = static_cast<const uint8_t *>(buf);
    if (bit_gw == 4) digest_rows<4>(b, pitch_bytes, r0, r1, grow0, pc0, lc0, ncols, slot);
    else if (bit_gw == 2) digest_rows<2>(b, pitch_bytes, r0, r1, grow0, pc0, lc0, ncols, slot);
    else digest_rows<0>(b, pitch_bytes, r0, r1, grow0, pc0, lc0, ncols, slot);
    return hipSuccess;
}
}  // namespace gol
