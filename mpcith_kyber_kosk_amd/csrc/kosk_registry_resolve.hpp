// The host half of an enrolment (kosk_registry_enrol*): duplicates within the call and the choice of slots.  Plain C++
// on public data (fingerprints, slot numbers, occupancy), no HIP: a stand-alone program can include and test it.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace kosk {

enum { ENROL_REJECTED = 0, ENROL_ADMITTED = 1, ENROL_DUPLICATE = 2 }; // KOSK_ENROL_* (kosk_capi.cpp asserts the equality)

// Positions in ascending b.  accept[b] == 0: REJECTED, slot -1, no occurrence of its key.  hit[b] >= 0 (the registry holds the fingerprint
// fp[b] in that slot) or fp[b] was ADMITTED at a lower position: DUPLICATE, the slot that holds the key.  Else ADMITTED into the
// lowest-numbered empty slot of occ not yet given out.  Returns the number of ADMITTED positions, or -1 when there are more new keys than
// empty slots (slots and status are then unspecified; the caller changes nothing)
inline int registry_enrol_resolve(int n, const uint8_t *accept, const uint8_t *fp, const int32_t *hit, const std::vector<uint8_t> &occ,
                                  std::vector<int32_t> &slots, std::vector<uint8_t> &status)
{
    slots.assign((size_t)n, -1);
    status.assign((size_t)n, (uint8_t)ENROL_REJECTED);
    std::map<std::array<uint8_t, 32>, int32_t> given; // fingerprints admitted by this call
    size_t next = 0;                                   // no empty slot below it is still free
    int admitted = 0;
    for (int b = 0; b < n; b++) {
        if (!accept[b]) continue;
        if (hit[b] >= 0) {
            slots[(size_t)b] = hit[b];
            status[(size_t)b] = (uint8_t)ENROL_DUPLICATE;
            continue;
        }
        std::array<uint8_t, 32> key;
        memcpy(key.data(), fp + (size_t)b * 32, 32);
        const auto it = given.find(key);
        if (it != given.end()) {
            slots[(size_t)b] = it->second;
            status[(size_t)b] = (uint8_t)ENROL_DUPLICATE;
            continue;
        }
        while (next < occ.size() && occ[next]) next++;
        if (next == occ.size()) return -1;
        given.emplace(key, (int32_t)next);
        slots[(size_t)b] = (int32_t)next++;
        status[(size_t)b] = (uint8_t)ENROL_ADMITTED;
        admitted++;
    }
    return admitted;
}

} // namespace kosk
