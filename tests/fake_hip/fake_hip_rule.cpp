// Host-only stand-in for the rule-generic launcher (test infrastructure, the
// companion of fake_hip.cpp: see its header).  Like every launch there it does
// nothing; gol_set_rule's argument checks and the schedule of a context with a
// rule set are what the CPU suite exercises (tests/test_rule_cpu.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {
bool bit_rule_supported(int gens, int gw) { return gw == 2 && gens >= 1 && gens <= 7; }
hipError_t launch_bit_rule(const StencilArgs &, int, const RuleMasks &, hipStream_t) { return hipSuccess; }
}  // namespace gol
