// launch_dispatch.hpp -- host side: from a workgroup size known at run time to a kernel instantiated for it, and the
// launch of a kernel that may ask for more dynamic LDS than the 48 KiB a kernel gets without saying so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include "device_views.hpp"   // namespace rdis_views, and its import into namespace rdis_hip

namespace rdis_views {

// f(std::integral_constant<int, T>) for the T of the list that equals `threads` -- for the LAST of the list when none does
// (every caller lists its default last).  All the calls of f must return the same type.
template <int T0, int... Ts, class F>
decltype(auto) with_threads(int threads, F&& f) {
    if constexpr (sizeof...(Ts) == 0) return f(std::integral_constant<int, T0>{});
    else if (threads == T0) return f(std::integral_constant<int, T0>{});
    else return with_threads<Ts...>(threads, static_cast<F&&>(f));
}

// kernel<<<grid, threads, dyn, stream>>>(args...), the kernel's dynamic-LDS limit raised first where dyn needs it
// (grid: a dim3, or an int for a grid of one dimension)
template <class... KA, class... A>
hipError_t launch_dyn(void (*kernel)(KA...), dim3 grid, int threads, size_t dyn, hipStream_t stream, const A&... args) {
    if (dyn > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        if (e != hipSuccess) return e;
    }
    kernel<<<grid, threads, dyn, stream>>>(args...);
    return hipGetLastError();
}

}  // namespace rdis_views
