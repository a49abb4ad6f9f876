// From run-time facts to template arguments, once, as plain host code (standard headers only, no HIP call:
// tests/native/dispatch_check.cpp compiles this file alone).  A launcher hands its body over as a generic lambda and reads the
// compile-time value off each tag it is called with: decltype(tag)::value.
//
// 1. The k-step counts of the MFMA kernels: KK = 2, 4, ..., 16 (MG_MAX_KK), four latent components per step.  THE statement of that set.
// 2. Booleans (latent dtype, output dtype, fused, split, score) as std::true_type / std::false_type.
#pragma once
#include <type_traits>
#include <utility>

template <int I> using mg_kk_tag = std::integral_constant<int, 2 * (I + 1)>;
using mg_kk_all = std::make_integer_sequence<int, 8>;

template <class R, class F, int... I>
inline R mg_dispatch_kk_in(int kk, R miss, F &f, std::integer_sequence<int, I...>) {
    (void)((kk == mg_kk_tag<I>::value && (miss = f(mg_kk_tag<I>{}), true)) || ...);
    return miss;
}
// f(std::integral_constant<int, KK>{}) for the KK that equals kk, and what it returns; `miss`, and no call, for any other kk
template <class R, class F>
inline R mg_dispatch_kk(int kk, R miss, F f) {
    return mg_dispatch_kk_in(kk, miss, f, mg_kk_all{});
}

template <class F, int... I>
inline int mg_each_kk_in(F &f, std::integer_sequence<int, I...>) {
    int rc = 0;
    (void)(((rc = f(mg_kk_tag<I>{})) == 0) && ...);
    return rc;
}
// f(tag) for every KK, ascending, as long as it returns 0 (MG_OK); the first other value, else 0
template <class F>
inline int mg_each_kk(F f) {
    return mg_each_kk_in(f, mg_kk_all{});
}

// f(tags...) with one std::true_type / std::false_type per flag, in argument order, and what it returns
template <class F>
inline auto mg_dispatch_flags(bool a, F f) {
    return a ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
inline auto mg_dispatch_flags(bool a, bool b, F f) {
    return mg_dispatch_flags(a, [&](auto A) { return mg_dispatch_flags(b, [&](auto B) { return f(A, B); }); });
}
template <class F>
inline auto mg_dispatch_flags(bool a, bool b, bool c, F f) {
    return mg_dispatch_flags(a, [&](auto A) { return mg_dispatch_flags(b, c, [&](auto B, auto C) { return f(A, B, C); }); });
}
