// Tuning switches of the dispatcher (host only: no HIP header; common.h includes this, gemm_route.cpp takes it alone).
#pragma once
#include <cstdlib>

namespace toist {

// The dispatcher's thresholds were found with environment switches (tools/dbg/ab_*.sh).  A product build compiles them to their
// defaults; `make KNOBS=1` (-DTOIST_TUNING_KNOBS) reads the environment once per process for A/B runs.
#ifdef TOIST_TUNING_KNOBS
inline long long tuning_knob(const char* name, long long dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoll(e) : dflt;
}
#else
inline long long tuning_knob(const char*, long long dflt) { return dflt; }
#endif

}  // namespace toist
