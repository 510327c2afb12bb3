// lanes.h -- how many lanes (internal streams + scratch sets, encoder.h) an encoder gets: host-only, no HIP, so that the rule can
// be checked without a GPU (tests/cpp/lanes_rule.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace fpng_amd {

// hw_queues: the hardware queues the library believes the HIP runtime uses (api.cpp runtime_defaults()); lanes_env: the value of
// FPNG_AMD_LANES, or null.  Four lanes over eight or more queues, else two (profiles/r05_hw_queues.txt); the variable overrides;
// always within 1 .. max_lanes.
inline uint32_t lanes_for(int hw_queues, const char *lanes_env, int max_lanes)
{
    const int n = lanes_env ? atoi(lanes_env) : (hw_queues >= 8 ? 4 : 2);
    return (uint32_t)std::min(std::max(n, 1), max_lanes);
}

} // namespace fpng_amd
