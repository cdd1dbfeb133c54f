// gol_view.h -- the tone map of a board view (include/gol/gol.h gol_view_tone), shared by the host entry point
// and the device kernel that maps view counts to Gray8 (gol_view.hip), so both compute the same pixel.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GOL_VIEW_HD __host__ __device__ __forceinline__
#else
#define GOL_VIEW_HD static inline
#endif

namespace gol {

constexpr int kViewAny = 0;      // GOL_VIEW_ANY
constexpr int kViewDensity = 1;  // GOL_VIEW_DENSITY
constexpr int64_t kViewMaxScale = 32768;              // a count fits uint32 (2^30 cells per pixel)
constexpr int64_t kViewMaxPixels = (int64_t)1 << 26;  // out_w * out_h

// count live cells of a pixel of scale x scale cells -> Gray8.  ANY: alive_value when any cell lives.  DENSITY:
// alive_value * count / n rounded half up, n = scale^2, in 64-bit.  Unknown modes and scales outside 1..32768 give 0.
GOL_VIEW_HD uint8_t view_tone(uint32_t count, int64_t scale, int mode, uint8_t alive_value) {
    if (scale < 1 || scale > kViewMaxScale) return 0;
    if (mode == kViewAny) return count ? alive_value : (uint8_t)0;
    if (mode != kViewDensity) return 0;
    const uint64_t n = (uint64_t)scale * (uint64_t)scale;
    const uint64_t t = (2 * (uint64_t)count * alive_value + n) / (2 * n);
    return (uint8_t)(t > 255 ? 255 : t);
}

}  // namespace gol
