// vs_dispatch.h -- how a launcher picks a kernel instantiation and launches it (host side).
//
// A kernel is a template over the rows' dtype, the metric and a few flags (QLDS: the query staged as fp64
// in LDS; SEL: rows taken from an id list).  dispatch() turns the runtime values into integral constants
// and hands them to a generic lambda, which names the kernel template once:
//
//     const bool known = dispatch(a.dt, a.metric, qlds, [&](auto dt, auto metric, auto qlds_c) {
//         launch_kernel(k_job<dt, metric, qlds_c>, LDS_DYN_MAX, grid, block, lds, st, a, ...);
//     });
//     return known ? hipGetLastError() : hipErrorInvalidValue;
//
// A launcher is its own argument checks plus one such call.  The LDS limits every launcher shares are here
// too: the dynamic-LDS limit and the budget a launcher fills before the query stays in global memory.
// (query_lds_bytes and pow2_at_least, the fp64 query's bytes and the power-of-two sizes of the LDS sorts, are in
// vs_internal.h, where the layout rules of host and device code see them.)
#pragma once
#include <tuple>
#include <type_traits>
#include <utility>

#include "vs_internal.h"

namespace vs {

constexpr int LDS_DYN_MAX = 152 << 10;        // the dynamic LDS limit a kernel is raised to (set_lds_attr)
constexpr size_t LDS_QUERY_BUDGET = 148 << 10;  // lists and query together: past it the query stays in global memory

template <int V>
using int_c = std::integral_constant<int, V>;

// fn(the dtype as an integral constant); false: the dtype has no kernel (F32 = false: fp32 rows have none)
template <bool F32 = true, class FN>
bool with_dt(int dt, FN&& fn) {
    if constexpr (F32) {
        if (dt == DT_F32) return fn(int_c<DT_F32>{}), true;
    }
    if (dt == DT_BF16) return fn(int_c<DT_BF16>{}), true;
    if (dt == DT_F16) return fn(int_c<DT_F16>{}), true;
    return false;
}

template <class FN>
bool with_metric(int metric, FN&& fn) {
    if (metric == METRIC_IP) return fn(int_c<METRIC_IP>{}), true;
    if (metric == METRIC_L2) return fn(int_c<METRIC_L2>{}), true;
    return false;
}

template <class FN>
bool with_bool(bool b, FN&& fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
    return true;
}

// (dispatch's tail: the constants chosen so far, then the bools still to choose, then fn)
template <class... C, class FN>
void dispatch_bools(std::tuple<C...>, FN&& fn) {
    fn(C{}...);
}
template <class... C, class... REST>
void dispatch_bools(std::tuple<C...>, bool b, REST&&... rest) {
    with_bool(b, [&](auto c) { dispatch_bools(std::tuple<C..., decltype(c)>{}, std::forward<REST>(rest)...); });
}

// dispatch(dt, metric, bools..., fn): fn(dt, metric, bools...), every one an integral constant;
// false (and fn not called): the dtype or the metric has no instantiation
template <bool F32 = true, class... REST>
bool dispatch(int dt, int metric, REST&&... rest) {
    bool known = false;
    with_dt<F32>(dt, [&](auto dt_c) {
        known = with_metric(metric, [&](auto metric_c) {
            dispatch_bools(std::tuple<decltype(dt_c), decltype(metric_c)>{}, std::forward<REST>(rest)...);
        });
    });
    return known;
}

// one launch: the kernel's dynamic LDS limit raised to lds_attr first (0: the default limit serves)
template <class KERNEL, class... ARGS>
void launch_kernel(KERNEL kernel, int lds_attr, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ARGS&... args) {
    if (lds_attr) set_lds_attr((const void*)kernel, lds_attr);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

}  // namespace vs
