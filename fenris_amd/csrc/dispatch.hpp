#pragma once
// Run-time value -> template argument, for the host launchers.  A launcher names the list of values that have an instantiation and says what
// happens for any other value; the generic lambda it passes gets the match as a std::integral_constant, so `k<v()>` names the kernel:
//
//     return dispatch(low_order_kinds, kind, -1, [&](auto ek) {            // -1: not covered, the caller falls back
//         return dispatch_or_last(solution_dims, S, [&](auto s) { ... k<ek(), s()> ...; return 0; });
//     });
//
// Only the combinations a lambda body names are instantiated: `if constexpr` inside it leaves out the pairs without a kernel.
#include <type_traits>

#include "../../include/fenris_hip.h"

namespace fenris_hip {

template <int... Vs> struct int_list {};

// f(integral_constant<V>) for the V of the list equal to v; `otherwise` when there is none
template <int V0, int... Vs, class R, class F>
auto dispatch(int_list<V0, Vs...>, int v, R otherwise, F&& f) {
    decltype(f(std::integral_constant<int, V0>{})) r = otherwise;
    (void)(((v == V0) ? (r = f(std::integral_constant<int, V0>{}), true) : false) || ... ||
           ((v == Vs) ? (r = f(std::integral_constant<int, Vs>{}), true) : false));
    return r;
}
// ... over two lists: f(integral_constant<V1>, integral_constant<V2>)
template <int... V1s, int... V2s, class R, class F>
auto dispatch(int_list<V1s...> l1, int v1, int_list<V2s...> l2, int v2, R otherwise, F&& f) {
    return dispatch(l1, v1, otherwise, [&](auto c1) { return dispatch(l2, v2, otherwise, [&](auto c2) { return f(c1, c2); }); });
}
// ... where every other value means the LAST entry of the list (the solution dimension: "not 1 or 2" is 3)
template <int... Vs, class F>
auto dispatch_or_last(int_list<Vs...>, int v, F&& f) {
    constexpr int vals[] = {Vs...};
    constexpr int last = vals[sizeof...(Vs) - 1];
    decltype(f(std::integral_constant<int, last>{})) r{};
    if (!((v == Vs ? (r = f(std::integral_constant<int, Vs>{}), true) : false) || ...)) r = f(std::integral_constant<int, last>{});
    return r;
}
template <class F>
auto dispatch_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// The recurring sets.  A new element kind or operator is added to the lists it has kernels for, here and nowhere else.
constexpr int_list<FH_QUAD4, FH_HEX8, FH_TET4, FH_HEX27, FH_TRI3, FH_TET10, FH_QUAD9, FH_TRI6, FH_HEX20, FH_TET20> all_kinds{};
constexpr int_list<FH_QUAD4, FH_HEX8, FH_TET4, FH_TRI3> low_order_kinds{};   // iso-parametric; the geometry kinds of all ten (Tri3 last: dispatch_or_last)
constexpr int_list<FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN, FH_STVK, FH_MASS_SCALAR, FH_MASS_VECTOR, FH_TENSOR, FH_STABLE_NEO_HOOKEAN> all_ops{};
constexpr int_list<FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN> elliptic_ops{};   // op_has_stress
constexpr int_list<FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN> hyperelastic_ops{};                              // op_depends_on_u
constexpr int_list<1, 2, 3> solution_dims{};
constexpr int_list<FH_RECOVER_GRAD_U, FH_RECOVER_STRAIN, FH_RECOVER_STRESS_PK1, FH_RECOVER_STRESS_CAUCHY, FH_RECOVER_VON_MISES,
                   FH_RECOVER_ENERGY_DENSITY, FH_RECOVER_VOLUME> recover_quantities{};
constexpr int_list<1, 2, 3, 4, 9> recover_components{};   // 1, d, d x s in two and three dimensions

// (D, NG) of an element kind: the dimension and the node count of its geometry
template <int EK>
struct kind_geom {
    static constexpr int D = (EK == FH_QUAD4 || EK == FH_TRI3 || EK == FH_QUAD9 || EK == FH_TRI6) ? 2 : 3;
    static constexpr int NG = (EK == FH_TRI3 || EK == FH_TRI6) ? 3 : (EK == FH_HEX8 || EK == FH_HEX27 || EK == FH_HEX20) ? 8 : 4;
};

}  // namespace fenris_hip
