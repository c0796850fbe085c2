// acm_dispatch.h on the host alone: every listed value reaches the lambda as exactly that constant, once, the lambda's status
// comes back, and a value outside a list gives ACM_NO_INSTANTIATION without a call, wherever the offending choice stands.
#include <cstdio>
#include <type_traits>
#include <initializer_list>

#include "acm_dispatch.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("dispatch_check: line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static_assert(std::is_same<decltype(acm_flag(true)), acm_choice<bool, false, true>>::value, "acm_flag is a choice of bool");
static_assert(ACM_NO_INSTANTIATION < -1, "distinct from a status (>= 0) and from the launchers' -1");

int main() {
    int calls = 0;
    // one choice
    for (int v : {1, 2, 3, 4, 6, 8, 10, 12}) {
        calls = 0;
        int seen = -1;
        const int rc = acm_pick([&](auto c) {
            static_assert(std::is_same<typename decltype(c)::value_type, int>::value, "an int constant");
            ++calls;
            seen = decltype(c)::value;
            return 100 + c();
        }, acm_one_of<1, 2, 3, 4, 6, 8, 10, 12>(v));
        CHECK(calls == 1 && seen == v && rc == 100 + v);
    }
    for (int v : {-1, 0, 5, 7, 13, 1 << 30}) {
        calls = 0;
        const int rc = acm_pick([&](auto) { ++calls; return 0; }, acm_one_of<1, 2, 3, 4, 6, 8, 10, 12>(v));
        CHECK(calls == 0 && rc == ACM_NO_INSTANTIATION);
    }
    // a flag is a bool constant: usable where a template takes bool, which an int constant is not
    for (bool b : {false, true}) {
        calls = 0;
        bool seen = !b;
        const int rc = acm_pick([&](auto f) {
            static_assert(std::is_same<decltype(f), std::bool_constant<decltype(f)::value>>::value, "a std::bool_constant");
            ++calls;
            seen = std::bool_constant<f()>::value;
            return 7;
        }, acm_flag(b));
        CHECK(calls == 1 && seen == b && rc == 7);
    }
    // two choices
    for (int a : {3, 4})
        for (bool b : {false, true}) {
            calls = 0;
            int sa = -1, sb = -1;
            const int rc = acm_pick([&](auto ca, auto cb) {
                ++calls;
                sa = decltype(ca)::value, sb = decltype(cb)::value;
                return 10 * ca() + cb();
            }, acm_one_of<3, 4>(a), acm_flag(b));
            CHECK(calls == 1 && sa == a && sb == (int)b && rc == 10 * a + (int)b);
        }
    // four choices, every cell
    for (int a : {3, 4})
        for (int b : {4, 8, 16})
            for (bool c : {false, true})
                for (bool d : {false, true}) {
                    calls = 0;
                    int s[4] = {-1, -1, -1, -1};
                    const int rc = acm_pick([&](auto ca, auto cb, auto cc, auto cd) {
                        ++calls;
                        s[0] = decltype(ca)::value, s[1] = decltype(cb)::value, s[2] = decltype(cc)::value, s[3] = decltype(cd)::value;
                        return ca() * 1000 + cb() * 10 + cc() * 2 + cd();
                    }, acm_one_of<3, 4>(a), acm_one_of<4, 8, 16>(b), acm_flag(c), acm_flag(d));
                    CHECK(calls == 1 && s[0] == a && s[1] == b && s[2] == (int)c && s[3] == (int)d);
                    CHECK(rc == a * 1000 + b * 10 + (int)c * 2 + (int)d);
                }
    // the value outside its list, in each of the four positions
    for (int pos = 0; pos < 4; ++pos) {
        int v[4] = {3, 8, 1, 6};
        v[pos] = 5;
        calls = 0;
        const int rc = acm_pick([&](auto, auto, auto, auto) { ++calls; return 0; }, acm_one_of<3, 4>(v[0]), acm_one_of<4, 8, 16>(v[1]),
                                acm_one_of<1, 2>(v[2]), acm_one_of<6, 12>(v[3]));
        CHECK(calls == 0 && rc == ACM_NO_INSTANTIATION);
    }
    for (int pos = 0; pos < 2; ++pos) {
        calls = 0;
        const int rc = acm_pick([&](auto, auto) { ++calls; return 0; }, acm_one_of<3, 4>(pos == 0 ? 5 : 3), acm_one_of<4, 8>(pos == 1 ? 5 : 8));
        CHECK(calls == 0 && rc == ACM_NO_INSTANTIATION);
    }
    // the lambda's own failure status is not mistaken for anything else
    CHECK(acm_pick([&](auto) { return 3; }, acm_one_of<1>(1)) == 3);
    if (failures) return 1;
    std::printf("dispatch_check: ok\n");
    return 0;
}
