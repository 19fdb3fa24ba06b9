// rt_format.h — the four RT_OUT_* formats, known here and nowhere else.  Validity, kind, size, the
// largest max_value and the kernel template for a run-time format are all read off this table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_mi355x.h"
#include "rt_pick.h"

// value: the format; type: the element of a frame; bits: the unsigned integer of the element's size
// (the slab codec moves bit patterns); max_value: the largest of an integer format (0: a float one)
template <int F, typename T, typename B, uint32_t MAXV>
struct rt_format_row {
    static constexpr int value = F;
    using type = T;
    using bits = B;
    static constexpr uint32_t max_value = MAXV;
};
template <int F>
struct rt_format;
template <> struct rt_format<RT_OUT_F64> : rt_format_row<RT_OUT_F64, double, uint64_t, 0> {};
template <> struct rt_format<RT_OUT_F32> : rt_format_row<RT_OUT_F32, float, uint32_t, 0> {};
template <> struct rt_format<RT_OUT_U8> : rt_format_row<RT_OUT_U8, uint8_t, uint8_t, 255> {};
template <> struct rt_format<RT_OUT_U16> : rt_format_row<RT_OUT_U16, uint16_t, uint16_t, RT_MAX_INT_VALUE> {};
static_assert(RT_OUT_F64 == 0 && RT_OUT_F32 == 1 && RT_OUT_U8 == 2 && RT_OUT_U16 == 3,
              "with_format walks the formats as the range [RT_OUT_F64, RT_OUT_U16]: floats first, then integers");

inline bool rt_format_ok(int precision) { return precision >= RT_OUT_F64 && precision <= RT_OUT_U16; }

// f(tag) for the format `precision` among [LO, HI] (all four; <RT_OUT_F64, RT_OUT_F32> the float
// ones, <RT_OUT_U8, RT_OUT_U16> the integer ones — only those are instantiated).  The tag is a
// value of rt_format<F>.  The caller has checked precision: one outside [LO, HI] is taken as HI.
template <int LO = RT_OUT_F64, int HI = RT_OUT_U16, typename Fn>
auto with_format(int precision, Fn &&f) {
    return with_int<LO, HI>(precision, [&](auto c) { return f(rt_format<decltype(c)::value>{}); });
}

inline size_t rt_elem_size(int precision) {
    return with_format(precision, [](auto t) { return sizeof(typename decltype(t)::type); });
}
// the largest max_value of an integer format: 255, or RT_MAX_INT_VALUE
inline uint32_t rt_max_value_of(int format) {
    return with_format(format, [](auto t) { return decltype(t)::max_value; });
}
// (both false for a value that is no format)
inline bool rt_is_int(int precision) { return rt_format_ok(precision) && rt_max_value_of(precision) != 0; }
inline bool rt_is_float(int precision) { return rt_format_ok(precision) && !rt_is_int(precision); }
