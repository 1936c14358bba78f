// Host build of csrc/ricci_otd_solve.h for tests/test_cpu_ricci_otd_solver.py: the solver source the kernels compile, run by one
// thread and by eight threads behind a barrier.  stdin: T, then per problem `na nb`, the na excesses, the nb deficits, the na * nb hop
// codes; stdout per problem: `W(1 thread) W(8 threads) rounds(1 thread) round_cap`.
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>
#define OTD_DEV inline
#include "ricci_otd_solve.h"

struct Problem { int na, nb; std::vector<long long> a, b; std::vector<unsigned> codes; };

template <int NT>
static long long run(const Problem& p, int* rounds) {
    std::vector<long long> a = p.a, b = p.b;
    std::vector<unsigned> x(p.na * p.nb);
    std::vector<unsigned short> pa(p.na), pb(p.nb);
    std::vector<unsigned char> sa(p.na), sb(p.nb);
    std::vector<signed char> qa(p.na), qb(p.nb);
    int sh[otd::SH_INTS];
    std::barrier bar(NT);
    std::mutex mu;
    long long w[NT];
    std::vector<std::thread> th;
    for (int t = 0; t < NT; ++t)
        th.emplace_back([&, t] {
            w[t] = otd::solve<NT, unsigned, long long>(p.codes.data(), p.na, p.nb, x.data(), a.data(), b.data(), pa.data(), pb.data(), sa.data(), sb.data(),
                                                        qa.data(), qb.data(), sh, t, [&] { bar.arrive_and_wait(); },
                                                        [&](int* q, int v) { std::lock_guard<std::mutex> g(mu); *q = std::min(*q, v); }, t == 0 ? rounds : nullptr);
        });
    for (auto& t : th) t.join();
    return w[0];
}

int main() {
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        Problem p;
        if (scanf("%d %d", &p.na, &p.nb) != 2) return 1;
        p.a.resize(p.na);
        p.b.resize(p.nb);
        for (auto& v : p.a) if (scanf("%lld", &v) != 1) return 1;
        for (auto& v : p.b) if (scanf("%lld", &v) != 1) return 1;
        p.codes.assign((p.na * p.nb + 15) / 16, 0u);
        for (int q = 0; q < p.na * p.nb; ++q) {
            int c;
            if (scanf("%d", &c) != 1 || c < 0 || c > 3) return 1;
            p.codes[q >> 4] |= (unsigned)c << ((q & 15) * 2);
        }
        int r1 = -1, r8 = -1;
        const long long w1 = run<1>(p, &r1), w8 = run<8>(p, &r8);
        printf("%lld %lld %d %d\n", w1, w8, r1, otd::round_cap(p.na, p.nb));
    }
    return 0;
}
