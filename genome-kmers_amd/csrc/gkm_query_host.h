// gkm_query_host.h -- how gk_lookup, gk_lookup_mismatch, gk_join, gk_screen, gk_match and gk_minimizers read
// their knobs.
// Plain C++ (no HIP): the stand-alone drivers run it under the host sanitizers (tests/sanitize).
#pragma once

#include <stdint.h>

#include <cstdlib>
#include <cstring>

namespace gkm {
namespace query {

// a GKM_*_PATH knob: 0 unset (the call chooses), 1 bytes, 2 keys, -1 any other value
constexpr int kPathBytes = 1, kPathKeys = 2;
inline int parse_path(const char *value) {
    if (!value) return 0;
    return std::strcmp(value, "bytes") == 0 ? kPathBytes : std::strcmp(value, "keys") == 0 ? kPathKeys : -1;
}

// a GKM_*_CHUNK knob (tests: several launches from a small batch): its decimal value when below def,
// else def -- nullptr / empty / 0 / not a number too.  A knob only lowers a default, never raises it,
// so the device scratch and the pinned staging stay bounded whatever its value.
inline uint64_t knob_below(const char *value, uint64_t def) {
    if (!value || !*value) return def;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(value, &end, 10);
    return end != value && *end == 0 && v != 0 && (uint64_t)v < def ? (uint64_t)v : def;
}

}  // namespace query
}  // namespace gkm
