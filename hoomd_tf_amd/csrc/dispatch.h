// Run-time values to compile-time constants, for the host side of a launch: a launch site hands its generic lambda to one of
// these and names its kernel and its arguments once, whatever the number of template switches.  Only the combinations a call
// can take are instantiated; a switch an entry fixes stays a literal in its lambda.
// Host translation units only: a generated unit (jit_unit.hip) sees neither this header nor <type_traits>.
#ifndef HTF_DISPATCH_H_
#define HTF_DISPATCH_H_
#include <type_traits>

namespace htf {

// f is called once with one std::true_type / std::false_type per flag, in the order given
template <typename F> inline void dispatch_flags(F &&f) { f(); }
template <typename F, typename... Bs> inline void dispatch_flags(F &&f, bool b, Bs... rest) {
    if (b) dispatch_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else   dispatch_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// f(std::integral_constant<int, V>{}) for the listed V equal to v; false, and no call, when v is not listed (a potential kind an
// entry does not accept, a precision, rows per wave, lanes per row, an epilogue level)
template <int... Vs, typename F> inline bool dispatch_value(F &&f, int v) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

template <bool F64> using scalar_t = std::conditional_t<F64, double, float>;   // a tensor's or the positions' scalar

} // namespace htf
#endif // HTF_DISPATCH_H_
