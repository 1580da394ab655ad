// Instrumentation (bench.py roofline): hipEvent pairs around sampled vsx_gemm_f16 launches.  prof.cpp holds the state and the
// vsx_prof_* entry points; the launch path brackets its launch with the two calls below.
#pragma once
#include "common.h"

namespace vsxg {

constexpr long PROF_NOT_SAMPLED = -1;
constexpr long PROF_FAILED = -2;        // an event could not be created (vsx_fail has the message): the launch returns VSX_E_LAUNCH

// Counts the launch and, when it is one to sample, records the opening event on `stream`.  Returns the sample's handle (>= 0),
// PROF_NOT_SAMPLED or PROF_FAILED.
long prof_begin(hipStream_t stream);
// Records the closing event of sample `handle` (>= 0) and books the launch's algorithmic FLOP and bytes.
void prof_end(long handle, hipStream_t stream, double flop, double bytes);

}  // namespace vsxg
