// gol_wave_dispatch.h -- the run-time shape of a wave-resident launch (NW = words per row 1..4, RPL = rows per lane
// 1..4, and the launcher's booleans) turned into template arguments, once, for gol_wave.hip, gol_batch.hip and
// gol_cycles.hip:
//
//   wave_dispatch([&](auto NW, auto RPL, auto BOUNDED, auto BYTES) { ... kernel<NW, RPL, BOUNDED, BYTES> ... },
//                 nw, rpl, bounded, bytes);
//
// calls the generic lambda with one std::integral_constant per value (each converts to its value in a constant
// expression) and returns what it returns; hipErrorInvalidValue where nw or rpl is out of range.  dispatch_planes does
// the same for the decay planes of a Generations launch, around it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace gol {

template <class F>
hipError_t dispatch_1to4(int n, F&& f) {
    switch (n) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
    }
    return hipErrorInvalidValue;
}

// (gol_generations.h gen_planes: 1..3 above 2 states)
template <class F>
hipError_t dispatch_planes(int planes, F&& f) {
    switch (planes) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
    }
    return hipErrorInvalidValue;
}

template <class F>
hipError_t dispatch_bools(F&& f) {
    return f();
}
template <class F, class... Bools>
hipError_t dispatch_bools(F&& f, bool b, Bools... rest) {
    if (b) return dispatch_bools([&](auto... c) { return f(std::true_type(), c...); }, rest...);
    return dispatch_bools([&](auto... c) { return f(std::false_type(), c...); }, rest...);
}

template <class F, class... Bools>
hipError_t wave_dispatch(F&& f, int nw, int rpl, Bools... bools) {
    return dispatch_1to4(nw, [&](auto NW) {
        return dispatch_1to4(rpl, [&](auto RPL) {
            return dispatch_bools([&](auto... c) { return f(NW, RPL, c...); }, bools...);
        });
    });
}

}  // namespace gol
