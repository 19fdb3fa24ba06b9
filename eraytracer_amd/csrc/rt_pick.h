// rt_pick.h — picking a kernel template on the host: a run-time value handed to a generic lambda as
// a compile-time constant (a std::integral_constant argument c; decltype(c)::value is the template
// argument).  Every helper returns what the lambda returns.
#pragma once
#include <type_traits>

#include "../../include/rt_mi355x.h"

template <typename F>
auto with_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
// v in [LO, HI] (a value above HI is taken as HI)
template <int LO, int HI, typename F>
auto with_int(int v, F &&f) {
    if constexpr (LO < HI) {
        if (v != LO) return with_int<LO + 1, HI>(v, f);
    }
    return f(std::integral_constant<int, LO>{});
}
// f(PREC, GENPOW): the output precision (RT_OUT_F64 / RT_OUT_F32) and whether the scene needs the general pow
template <typename F>
auto with_prec_pow(int precision, bool int_pow, F &&f) {
    return with_int<RT_OUT_F64, RT_OUT_F32>(precision, [&](auto prec) {
        return with_bool(!int_pow, [&](auto genpow) { return f(prec, genpow); });
    });
}
