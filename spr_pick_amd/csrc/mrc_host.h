// The MRC sample types on the host: the mode check, the step from a mode to its sample type and the anchor check that the
// entry points reading raw samples share.  Not part of the ABI.
#pragma once
#include <cstdint>
#include <limits>
#include <type_traits>

#include "common.h"

namespace {

inline bool mrc_mode_ok(int mode) {
    return mode == SPRK_MRC_INT8 || mode == SPRK_MRC_INT16 || mode == SPRK_MRC_FLOAT32 || mode == SPRK_MRC_UINT16;
}
// `who`: the entry point's name, as a string literal
#define SPRK_REQUIRE_MRC_MODE(who, mode) \
    SPRK_REQUIRE(mrc_mode_ok(mode), who ": unsupported MRC mode %d (0, 1, 2 and 6 are)", mode)

// f(tag) with a value-initialised object of the sample type of `mode` (checked before: any other mode goes as uint16)
template <typename F>
auto dispatch_mrc(int mode, F &&f) {
    switch (mode) {
        case SPRK_MRC_INT8: return f(int8_t{});
        case SPRK_MRC_INT16: return f(int16_t{});
        case SPRK_MRC_FLOAT32: return f(float{});
        default: return f(uint16_t{});
    }
}

// the anchor of an integer mode is a sample value (the kernels subtract it in integers); float32 has none
template <typename T>
bool anchor_is_sample(float anchor) {
    return anchor >= (float)std::numeric_limits<T>::min() && anchor <= (float)std::numeric_limits<T>::max() &&
           (float)(T)anchor == anchor;
}
inline bool anchor_ok(int mode, float anchor) {
    return dispatch_mrc(mode, [&](auto tag) {
        using T = decltype(tag);
        if constexpr (std::is_same<T, float>::value) return anchor == 0.0f;
        else return anchor_is_sample<T>(anchor);
    });
}

}  // namespace
