// test_gen_board.cpp -- the host-side pieces of Generations rules on a single board, a program of its
// own under the address and undefined-behaviour sanitizers (tests/test_board_generations_host.py builds and runs it):
//   1. the cell conversion of the state I/O kernels (gen_cell_convert) round-tripped for every state of every nstates;
//   2. the depth table gen_stream_max_k (csrc/gol_gen_plan.h): 4, 2 or 1 everywhere, never rising with the planes;
//   3. a scalar model of one level of gol_gen_stream with its decay planes -- a row's decay words stored at window slot
//      t % 3 are the ones gen_decay meets one step later with that row's alive words -- against gen_next_cell on a
//      column of rows one word wide.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <random>

#include "../../gameoflifewithactors_amd/csrc/gol_gen_plan.h"
#include "../../gameoflifewithactors_amd/csrc/gol_generations.h"

using namespace gol;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            if (++failures > 20) exit(1);                          \
        }                                                          \
    } while (0)

static int conversions() {
    int n = 0;
    for (int nstates = kGenStatesMin; nstates <= kGenStatesMax; nstates++)
        for (int s = 0; s < nstates; s++, n++) {
            int in = s, out = -1;
            uint32_t alive = 77, d = 77;
            gen_cell_convert(false, in, alive, d);
            CHECK(in == s && alive == (s == 1 ? 1u : 0u) && d == (s >= 2 ? (uint32_t)(s - 1) : 0u));
            CHECK(!(alive && d) && d <= (uint32_t)(nstates - 2 > 0 ? nstates - 2 : 0));  // exclusive, d in 1 .. C - 2
            CHECK(d < (1u << gen_planes(nstates)));                                      // d fits the planes
            gen_cell_convert(true, out, alive, d);
            CHECK(out == s);
        }
    return n;
}

static int depths() {
    int n = 0;
    for (int ilv : {1, 2, 4})
        for (int bounded = 0; bounded < 2; bounded++) {
            int last = 8;
            for (int planes = 1; planes <= kGenPlanesMax; planes++, n++) {
                const int k = gen_stream_max_k(ilv, planes, bounded != 0);
                CHECK(k == 4 || k == 2 || k == 1);
                CHECK(k <= last);
                last = k;
                for (int left = 1; left <= 9; left++) {  // the chunks of a call: depths of the table, summing to it
                    int done = 0, steps = 0;
                    while (done < left && steps++ < 16) {
                        const int g = gen_stream_largest_k(left - done, k);
                        CHECK((g == 4 || g == 2 || g == 1) && g <= k && g <= left - done);
                        done += g;
                    }
                    CHECK(done == left);
                }
            }
        }
    CHECK(gen_stream_max_k(3, 1, false) == 0 && gen_stream_max_k(1, 0, false) == 0 && gen_stream_max_k(1, 4, true) == 0);
    return n;
}

// One level of the pass on a column of `rows` rows of one word (32 cells; no cell beside the word, none above row 0 or
// below the last): the window's three slots as the kernel has them, rotating by t % 3.
template <int P>
static int level_model(std::mt19937& rng, int nstates, int birth, int survive) {
    constexpr int kRows = 12;
    int st[kRows][32];
    for (auto& row : st)
        for (int& c : row) c = (int)(rng() % (unsigned)nstates);
    uint32_t s[3][1] = {}, c[3][1] = {}, a[3][1] = {}, d[3][P] = {};
    const GenMasks g = gen_masks(nstates);
    const uint32_t rule = rule_pack(birth, survive);
    int checked = 0;
    for (int t = 0; t <= kRows; t++) {  // step t: row t enters (a row of zeros after the last), row t - 1 is finished
        const int PH = t % 3, PV = (t + 1) % 3, C = (t + 2) % 3;
        uint32_t x[1] = {0}, dx[P];
        for (int k = 0; k < P; k++) dx[k] = 0;
        if (t < kRows)
            for (int b = 0; b < 32; b++) {
                int sv = st[t][b];
                uint32_t al, dd;
                gen_cell_convert(false, sv, al, dd);
                x[0] |= al << b;
                for (int k = 0; k < P; k++) dx[k] |= (dd >> k & 1u) << b;
            }
        row_sum_block<1>(x, 0u, 0u, s[PH], c[PH]);
        a[PH][0] = x[0];
        for (int k = 0; k < P; k++) d[PH][k] = dx[k];
        uint32_t v[1];
        rule_next_row<1>(s[PV], c[PV], s[C], c[C], s[PH], c[PH], a[C], rule, v);
        uint32_t dd[P];
        for (int k = 0; k < P; k++) dd[k] = d[C][k];
        const uint32_t an = gen_decay<P>(a[C][0], v[0], dd, g);
        if (t == 0) continue;  // nothing finished yet
        const int y = t - 1;
        for (int b = 0; b < 32; b++, checked++) {
            int n = 0;
            for (int dy = -1; dy <= 1; dy++)
                for (int db = -1; db <= 1; db++) {
                    if (!dy && !db) continue;
                    const int yy = y + dy, bb = b + db;
                    if (yy < 0 || yy >= kRows || bb < 0 || bb >= 32) continue;
                    n += st[yy][bb] == 1;
                }
            uint32_t al = an >> b & 1u, dv = 0;
            for (int k = 0; k < P; k++) dv |= (dd[k] >> b & 1u) << k;
            int got = -1;
            gen_cell_convert(true, got, al, dv);
            CHECK(!(al && dv));
            CHECK(got == gen_next_cell(st[y][b], n, birth, survive, nstates));
        }
    }
    return checked;
}

int main() {
    printf("cell conversion: %d states\n", conversions());
    printf("depth table: %d entries\n", depths());
    std::mt19937 rng(20240607);
    long cells = 0;
    for (int nstates = 3; nstates <= kGenStatesMax; nstates++)
        for (int r = 0; r < 40; r++) {
            const int birth = r == 0 ? 0x1FF : (int)(rng() & 0x1FF), survive = r == 1 ? 0x1FF : (int)(rng() & 0x1FF);
            switch (gen_planes(nstates)) {
                case 1: cells += level_model<1>(rng, nstates, birth, survive); break;
                case 2: cells += level_model<2>(rng, nstates, birth, survive); break;
                case 3: cells += level_model<3>(rng, nstates, birth, survive); break;
            }
        }
    printf("level model: %ld cells\n", cells);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("gen board ok\n");
    return 0;
}
