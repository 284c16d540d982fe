// f(integral_constant<int, I>) ... f(integral_constant<int, N - 1>): a loop whose index is a compile-time constant in its body
#pragma once
#include <type_traits>

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
