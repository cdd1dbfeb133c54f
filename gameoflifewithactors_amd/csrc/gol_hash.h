// gol_hash.h -- the two 64-bit mixers the project's definitions name ("Canonical hash" and "Large-board
// init"), host + gfx950 device: fmix64 (MurmurHash3's finaliser) under the board hash, splitmix64 under the splitmix
// seeding.  No HIP here beyond gol_bitlogic.h's host/device marker.
#pragma once
#include <stdint.h>

#include "gol_bitlogic.h"

namespace gol {

GOL_HD uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

GOL_HD uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

}  // namespace gol
