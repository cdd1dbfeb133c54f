// Host-only check of csrc/gol_cycle_search.h (the control flow of gol_ensemble_cycles), with its own main.  Built with
// -fsanitize=address,undefined by tests/test_cycles_host.py.  The state is a position on the rho sequence x_0 ..
// x_{mu+lambda-1} distinct, then back to x_mu; every 0 <= mu <= 40, 1 <= lambda <= 40, 1 <= G <= 90 is searched and
// compared with the definition: resolved exactly when mu + lambda <= G, exact mu and lambda then, (-1, 0) otherwise,
// and never more than 6 G steps.
#include <cstdio>
#include <cstdlib>

#include "../../gameoflifewithactors_amd/csrc/gol_cycle_search.h"

#define CHECK(c)                                                                                               \
    do {                                                                                                       \
        if (!(c)) {                                                                                            \
            std::printf("%s:%d: %s failed (mu %d lambda %d G %d: got %d %d, %d steps)\n", __FILE__, __LINE__, #c, mu, \
                        lambda, G, (int)r.transient, (int)r.period, (int)r.steps);                             \
            std::exit(1);                                                                                      \
        }                                                                                                      \
    } while (0)

namespace {

long g_steps = 0;  // counted here too: the header's own count must agree

struct Rho {
    int mu, lambda, pos;
    void step() {
        pos = pos + 1 == mu + lambda ? mu : pos + 1;
        g_steps++;
    }
    bool equal(const Rho& o) const { return pos == o.pos; }
};

}  // namespace

int main() {
    long cases = 0, resolved = 0, worst_num = 0, worst_den = 1;
    for (int mu = 0; mu <= 40; mu++)
        for (int lambda = 1; lambda <= 40; lambda++)
            for (int G = 1; G <= 90; G++) {
                g_steps = 0;
                int hits = 0, hit_pos = -1;
                const gol::CycleResult r = gol::cycle_search<Rho>([&] { return Rho{mu, lambda, 0}; }, G,
                                                                  [&](const Rho& a) { hits++, hit_pos = a.pos; });
                CHECK(r.steps == g_steps);
                CHECK(r.steps >= 0 && r.steps <= 6 * G);
                if (mu + lambda <= G) {
                    CHECK(r.transient == mu && r.period == lambda);
                    CHECK(hits == 1 && hit_pos == mu);  // the state handed over is x_mu
                    resolved++;
                } else {
                    CHECK(r.transient == -1 && r.period == 0);
                    CHECK(hits == 0);
                }
                if (r.steps * worst_den > worst_num * G) worst_num = r.steps, worst_den = G;
                cases++;
            }
    const int big = 1 << 20;
    // G outside 1 .. 2^20 is refused without a step
    const int refused[3] = {0, -1, big + 1};
    for (int G : refused) {
        const int mu = 0, lambda = 1;
        g_steps = 0;
        const gol::CycleResult r = gol::cycle_search<Rho>([&] { return Rho{mu, lambda, 0}; }, G, [](const Rho&) {});
        CHECK(r.transient == -1 && r.period == 0 && r.steps == 0 && g_steps == 0);
    }
    // the largest G: no counter overflows at the longest transient, the longest period, one past either, or with a
    // fixed point found at once
    const int extremes[5][3] = {{0, 1, 2}, {big - 1, 1, 0}, {0, big, 0}, {big, 1, 0}, {0, big + 1, 0}};
    for (const auto& e : extremes) {
        const int mu = e[0], lambda = e[1], G = big;
        g_steps = 0;
        const gol::CycleResult r = gol::cycle_search<Rho>([&] { return Rho{mu, lambda, 0}; }, G, [](const Rho&) {});
        CHECK(r.steps == g_steps && r.steps <= 6 * (long)G);
        if (mu + lambda <= G)
            CHECK(r.transient == mu && r.period == lambda);
        else
            CHECK(r.transient == -1 && r.period == 0);
        if (e[2]) CHECK(r.steps == e[2]);
    }
    std::printf("cycle search ok: %ld cases, %ld resolved, most steps %ld at G = %ld\n", cases, resolved, worst_num,
                worst_den);
    return 0;
}
