// What the entry points of K4 (mu_temporal.hip) and K4h (hals_temporal.hip) share: the argument checks, the choice of the list
// width, and (warp_gram_lists.hpp) the reader of K3n's slot tables.
#pragma once

#include <type_traits>

#include "warp_gram_lists.hpp"

namespace dnmf {

// which forms of G a call has: the dense one only, lists of NN columns a row only, or both (NN = 0: dense)
enum TraceLists { DENSE_ONLY, LISTS_ONLY, LISTS_OR_DENSE };

// K, T and ldc, with `more_ok` the condition on the call's further arguments and `more` (printf-style) their text; then what is
// built: K <= 256, NN in {8, 16, 32}.  Every message starts with the call's name `fn`.
inline int check_trace_call(const char *fn, int K, int T, long ldc, TraceLists lists, int NN, bool more_ok, const char *more, ...) {
    if (!(K > 0 && T > 0 && ldc >= T && more_ok)) {
        char text[96];
        va_list ap;
        va_start(ap, more);
        vsnprintf(text, sizeof text, more, ap);
        va_end(ap);
        return fail(DNMF_E_SHAPE, "%s: K=%d T=%d ldc=%ld%s", fn, K, T, ldc, text);
    }
    if (lists == DENSE_ONLY) {
        DNMF_REQUIRE(K <= 256, DNMF_E_UNSUPPORTED, "%s: K=%d > 256 (not built yet)", fn, K);
    } else {
        DNMF_REQUIRE(K <= 256 && ((lists == LISTS_OR_DENSE && NN == 0) || NN == 8 || NN == 16 || NN == 32), DNMF_E_UNSUPPORTED,
                     "%s: K=%d (<= 256), NN=%d (8, 16 or 32%s)", fn, K, NN, lists == LISTS_OR_DENSE ? " with nbr" : "");
    }
    return DNMF_OK;
}

// f(std::integral_constant<int, NN>{}) for the NN that check_trace_call let through: 8, 16, 32, and with DENSE also 0
template <bool DENSE, typename F>
inline void with_list_width(int NN, F f) {
    using std::integral_constant;
    if constexpr (DENSE) {
        if (NN == 0) return f(integral_constant<int, 0>{});
    }
    if (NN == 8) f(integral_constant<int, 8>{});
    else if (NN == 16) f(integral_constant<int, 16>{});
    else f(integral_constant<int, 32>{});
}

}  // namespace dnmf
