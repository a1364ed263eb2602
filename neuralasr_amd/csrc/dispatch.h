// dispatch.h — host: a run-time value picks a template argument (the launchers of lstm*.hip and ctc.hip).
#pragma once
#include <type_traits>
#include <utility>

namespace nasr {

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; the LAST value of the list is the default
template <class F, int V0, int... Vs>
inline void dispatch_int(std::integer_sequence<int, V0, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) {
    f(std::integral_constant<int, V0>{});
  } else {
    if (v == V0) f(std::integral_constant<int, V0>{});
    else dispatch_int(std::integer_sequence<int, Vs...>{}, v, f);
  }
}
// f for every value of the list
template <class F, int... Vs>
inline void for_each_int(std::integer_sequence<int, Vs...>, F&& f) {
  (f(std::integral_constant<int, Vs>{}), ...);
}

}  // namespace nasr
