// weasal_amd/csrc/ws_dispatch.h -- a plan's runtime values onto template arguments: the one idiom of every launcher.
//
// dispatch(f, Pick<1, 2, 4>{v}, ...) calls f with one std::integral_constant per Pick: the value of its list that equals v.
// It returns whether f was called: a value outside a list launches nothing, and the launcher turns `false` into an error
// that names the plan.  What a kernel family does not instantiate is pruned with if constexpr at the launch.  The row type
// is one more Pick: Flag{p.bf16} -> Row<bf.value>.  A plan value that is a threshold (c <= 4 / 8 / 12 ...) is mapped to the
// instantiated value first, and that value is picked.
#pragma once
#include <type_traits>
#include "ws_common.h"
#include "ws_bf16.h"

template <int... Vs> struct Pick { int v; };
using Flag = Pick<0, 1>;
template <typename F> bool dispatch(F&& f) { f(); return true; }
template <typename F, int... Vs, typename... Rest>
bool dispatch(F&& f, Pick<Vs...> a, Rest... rest)
{
    return (((a.v == Vs) && dispatch([&](auto... cs) { f(std::integral_constant<int, Vs>{}, cs...); }, rest...)) || ...);
}
template <int BF> using Row = std::conditional_t<BF != 0, bf16_t, float>;

// what a launcher returns when dispatch matched nothing, e.g. ws_no_instantiation("gemm_xb2_kernel<NT=%d, WN=%d>", p.nt, p.wn)
__attribute__((format(printf, 1, 2))) inline int ws_no_instantiation(const char* fmt, ...)
{
    char plan[192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(plan, sizeof plan, fmt, ap);
    va_end(ap);
    return ws_fail(WS_ERR_UNSUPPORTED, "%s: the plan names an instantiation that does not exist", plan);
}
