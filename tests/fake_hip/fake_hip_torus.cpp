// Host-only stand-ins for the GOL_TORUS launchers (test infrastructure, the
// companion of fake_hip.cpp: see its header).  Like every launch there they do
// nothing; the runtime's schedule around them — the wrap after every stencil
// launch, the halo ring — is what the CPU suite records and race-checks
// (tests/test_torus_cpu.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {
hipError_t launch_wrap_cols(void *, int64_t, int64_t, int64_t, int64_t, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_interleave_rows_shift(const uint32_t *, uint32_t *, int64_t, int64_t, int64_t, int64_t, int64_t, int,
                                        int, hipStream_t) {
    return hipSuccess;
}
hipError_t launch_popcount_cols(const void *, int64_t, int64_t, int64_t, int64_t, int64_t, unsigned long long *, int,
                                hipStream_t) {
    return hipSuccess;
}
}  // namespace gol
