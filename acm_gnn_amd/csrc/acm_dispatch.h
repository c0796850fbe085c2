// Host side: the one translation from runtime values to kernel template arguments.
//
//     acm_pick([&](auto nc, auto ln) {
//         hipLaunchKernelGGL((kernel<nc(), ln()>), grid, block, 0, st, args...);
//         return ACM_OK;
//     }, acm_one_of<3, 4>(NC), acm_flag(layernorm != 0));
//
// calls the lambda once, with one std::integral_constant per choice, and returns the lambda's int status.  A value that
// is not in its list gives ACM_NO_INSTANTIATION without a call: there is no default arm.
#pragma once
#include <type_traits>

// not an acm_status_t, and not the -1 / 0 some launchers return for "not this kernel"
constexpr int ACM_NO_INSTANTIATION = -0x7fffffff;

template <typename T, T... Vs>
struct acm_choice {
    T v;
};
template <int... Vs>
constexpr acm_choice<int, Vs...> acm_one_of(int v) {
    return {v};
}
constexpr acm_choice<bool, false, true> acm_flag(bool b) {
    return {b};
}

template <typename F>
int acm_pick(F&& f) {
    return f();
}
template <typename F, typename T, T... Vs, typename... Rest>
int acm_pick(F&& f, acm_choice<T, Vs...> c, Rest... rest) {
    int r = ACM_NO_INSTANTIATION;
    // at most one value matches; the fold stops there
    (void)((c.v == Vs && (r = acm_pick([&](auto... cs) { return f(std::integral_constant<T, Vs>{}, cs...); }, rest...), true)) || ...);
    return r;
}
